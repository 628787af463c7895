// attention_bwd_panels.hip — fused sparse attention backward for gfx950 on matrix instructions, per
// 16-row and per 16-column panel (bsmr_attention_backward_panels; fp16 / bf16 operands, D and Dv
// each 32, 64 or 128). The definition is bsmr_attention_backward's (attention_bwd.hip):
//
//   GQ[i,:] = sum_e dp_e K[j_e,:]   GK[j,:] = sum_{e in column j} dp_e Q[i_e,:]   GV[j,:] = sum w_e GO[i_e,:]
//   x = p scale, w = 2^((x - LSE_i) log2e) (0 when LSE_i = -inf), dp = (w (g - delta_i)) scale
//
// with p = dot(Q[i], K[j]) and g = dot(GO[i], V[j]) out of v_mfma_f32_16x16x32_{f16,bf16}. LSE holds
// every row's shift, so there is no running maximum, no rescale of an accumulator, and a split
// panel's items add by plain sums. Lane l = (r, g) = (l & 15, l >> 4) as in attention_panels.hip
// (panel_mfma.hpp). At most five launches:
//   k_attention_bwd_delta (attention_bwd.hip, unchanged): delta, slices x M floats of this path's own;
//   k_attention_bwd_panels_rows: a wave per item of the forward's lists (<= 16 steps of 32 columns of
//     a row panel's column union). For the whole item lane (r, g) keeps Q[row r][32 s + 8 g, +8),
//     GO[row r][32 s + 8 g, +8) rounded once to the operand type (two 16-byte loads and four packs
//     per 8), LSE_r and delta_r. Per step: S^T = K_tile Q^T and G^T = V_tile GO^T, the A operands
//     16-byte global loads of the K and V rows requested one step ahead, so lane (r, g) holds p and
//     g of its own row at step columns 4 g + j and 16 + 4 g + j; w and dp in fp32, +0 by a select
//     where the row does not store the column; dp rounded to the operand type as the B operand of
//     dQ^T += K^T dp^T, whose A operands are the step's 32 K rows staged in LDS (the word + permute
//     read, rows 2 D + 16 bytes apart). The first product keeps the forward's own global read of
//     the K rows (a second read, from L2) rather than the stage: its operands are then in flight a
//     step ahead, which the staged rows cannot be without a second LDS buffer. Lane (r, g) ends
//     with GQ[row r][32 n + 8 g, +8);
//   k_attention_bwd_panels_cols: a wave per item of the same kind of lists of the transposed pattern
//     (<= 16 steps of 32 union ROWS of 16 consecutive columns). For the item lane (c, g) keeps
//     K[col c] and V[col c] as B operands. Per step the 32 Q rows (as loaded) and the 32 GO rows
//     (rounded once, in the operand type) are staged in LDS, 32 (2 D + 16) + 32 (2 Dv + 16) bytes;
//     S = Q_tile K^T and G = GO_tile V^T take their A operands from the stage by 16-byte reads (one
//     global load of every Q and GO row per step; 16 lanes of such a read cover all 64 banks), so
//     lane (c, g) holds p and g of its column at step rows 4 g + j and 16 + 4 g + j; LSE and delta
//     of the step's rows are loaded one per lane and handed out by shuffle; then
//     dV^T += GO^T w^T and dK^T += Q^T dp^T from the stage by the word + permute read;
//   k_attention_bwd_panels_reduce after either: a split panel's partial slots (16 rows each) added
//     in item order, GK and GV in one launch.
// No atomics; the summation order is a function of the panel unions alone.
//
// Conventions: bsmr_attention_backward's, with GO, w and dp rounded once to the operand type before
// they enter an MFMA (fp16: |GO| or |dp| above 65504 becomes inf), and what 0 x NaN inside an MFMA
// does to a row staged for a second product: a NaN / inf in K[j] reaches the GQ rows of the row
// panels whose union holds j, one in Q[i] or GO[i] the GK / GV rows of the column panels whose
// union holds i, and no other destination. 256 is left out: at D = Dv = 256 the columns side would
// hold K, V and the two accumulators in 32 + 32 + 64 + 64 registers before an operand is in flight.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "attention_common.hpp"
#include "attention_layout.hpp"
#include "attention_panels.hpp"
#include "attention_panels_args.hpp"  // attn_panels_check_bias
#include "panel_host.hpp"
#include "panel_mfma.hpp"
#include "plan.hpp"
#include "seg_walk.hpp"  // exp2_hw

namespace bsmr {
namespace {

constexpr float LOG2E_F = 1.44269504088896340736f;

struct BwdPanelArgs {
    const PanelItem* items;
    const PanelStep* steps;
    const u32* rows;         // rows side: the launch order; columns side: null (column = position)
    AttnOpBytes Q, K, V;     // strides in bytes, 2-byte elements
    AttnOpBytes GO;          // fp32
    const float* lse;        // slices x M
    const float* delta;      // slices x M
    AttnOpBytes Y0, Y1;      // rows side: GQ, -; columns side: GK, GV (either may be null)
    float* P0;               // slices x partials x 16 x D
    float* P1;               // columns side: behind them, slices x partials x 16 x Dv
    u32 partials, heads, M, nDst, nItems;  // nDst: M on the rows side, N on the columns side
    float scale;
    // the BIAS instantiations only (null / 0 elsewhere): the side's entry positions (spmm_panels.hpp:
    // on the columns side the CSR index carried through the transpose), the bias and, on the rows
    // side, GBias (null: not asked for), nnz fp32 values at CSR positions per slice, with their
    // slice strides in elements (bias: 0 is one for all slices)
    const u32* base;
    const u32* pos;
    const float* bias;
    float* gbias;
    u64 biasStride, gbiasStride;
};

constexpr u32 NO_ENTRY = 0xFFFFFFFFu;  // the position of a slot whose mask bit is clear

// attention_bwd.hip's weight_of, every product and difference rounded on its own, and then the
// forward's rule: exactly +0 where the entry is not stored, whatever the products were
template <bool BIAS = false>
__device__ __forceinline__ void panel_weight(float p, float g, float lse, float dl, float scale, bool stored, float& w,
                                             float& dp, float b = 0.f, float* h = nullptr) {
#pragma clang fp contract(off)
    float x = p * scale;
    if constexpr (BIAS) x = x + b;  // (the biased form's x: the sum rounded on its own)
    const float d = x - lse;
    const float t = d * LOG2E_F;
    const float wv = lse == -INFINITY ? 0.f : exp2_hw(t);
    const float gd = g - dl;
    const float wg = wv * gd;
    const float dv = wg * scale;
    w = stored ? wv : 0.f;
    dp = stored ? dv : 0.f;
    if constexpr (BIAS) *h = wg;  // GBias of a stored entry
}

// The biased form's gather (attention_panels_bias.hip): the positions of destination d's entries at
// the lane's eight step slots, pos[base[d] + popcount(mask_d below the slot)], and the bias there;
// each load predicated on the mask bit
__device__ __forceinline__ void bias_positions(const u32* pos, u32 mask, u32 b, u32 g, u32* p) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const u32 c = panel_slot(g, j);
        p[j] = NO_ENTRY;
        if ((mask >> c) & 1u) p[j] = pos[b + __builtin_popcount(mask & ((1u << c) - 1u))];
    }
}
__device__ __forceinline__ void bias_values(const float* bias, const u32* p, float* w) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        w[j] = 0.f;
        if (p[j] != NO_ENTRY) w[j] = bias[p[j]];
    }
}

// eight consecutive fp32 elements rounded once to the operand type
template <int DT>
__device__ __forceinline__ uint4 load8_rounded(const char* p) {
    const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 16);
    return make_uint4(pack2<DT>(lo.x, lo.y), pack2<DT>(lo.z, lo.w), pack2<DT>(hi.x, hi.y), pack2<DT>(hi.z, hi.w));
}

template <int DT, int D, int DV, bool BIAS>
__global__ __launch_bounds__(PANEL_WAVES * 64) __attribute__((amdgpu_waves_per_eu(2)))
void k_attention_bwd_panels_rows(const BwdPanelArgs a) {
    constexpr int KS = D / 32;                 // k-steps of a score tile, and pairs of GQ tiles
    constexpr int VS = DV / 32;                // k-steps of a g tile
    constexpr u32 KROW = staged_row_bytes(D);  // bytes between staged K rows
    constexpr u32 CPR = D / 8;                 // 16-byte chunks per K row
    constexpr int KLOADS = D / 16;             // chunks per lane and step (32 rows)
    __shared__ __attribute__((aligned(16))) char kstage[PANEL_WAVES][PANEL_STEP_COLS * KROW];

    const u32 lane = threadIdx.x & 63u;
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 itemId = blockIdx.x * PANEL_WAVES + wave;
    if (itemId >= a.nItems) return;
    const PanelItem it = a.items[itemId];
    const u32 head = blockIdx.y, bat = blockIdx.z;
    const size_t slice = static_cast<size_t>(bat) * a.heads + head;
    const char* Qs = attn_slice_base(a.Q, bat, head);
    const char* Ks = attn_slice_base(a.K, bat, head);
    const char* Vs = attn_slice_base(a.V, bat, head);
    const char* GOs = attn_slice_base(a.GO, bat, head);
    char* kl = kstage[wave];

    const u32 r = lane & 15u, g = lane >> 4;
    const bool live = it.row0 + r < a.M;  // (a row of a short last panel is neither loaded nor stored)
    const u32 row = live ? a.rows[it.row0 + r] : 0u;
    uint4 q[KS], go[VS];
    panel_row_operand(q, Qs + static_cast<size_t>(row) * a.Q.row, live, g);
#pragma unroll
    for (int s = 0; s < VS; ++s)
        go[s] = live ? load8_rounded<DT>(GOs + static_cast<size_t>(row) * a.GO.row + (32u * s + 8u * g) * 4u)
                     : make_uint4(0, 0, 0, 0);
    const float lse = live ? a.lse[slice * a.M + row] : 0.f;
    const float dl = live ? a.delta[slice * a.M + row] : 0.f;

    f32x4 acc[2 * KS];
#pragma unroll
    for (int n = 0; n < 2 * KS; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

    const PanelStep* st = a.steps + it.step0;
    uint4 k0[KS], k1[KS], v0[VS], v1[VS];
    auto load_kv = [&](const PanelStep* sp) {
        const u32 c0 = sp->cols[r], c1 = sp->cols[16u + r];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            k0[s] = load16(Ks + static_cast<size_t>(c0) * a.K.row + (32u * s + 8u * g) * 2u);
            k1[s] = load16(Ks + static_cast<size_t>(c1) * a.K.row + (32u * s + 8u * g) * 2u);
        }
#pragma unroll
        for (int s = 0; s < VS; ++s) {
            v0[s] = load16(Vs + static_cast<size_t>(c0) * a.V.row + (32u * s + 8u * g) * 2u);
            v1[s] = load16(Vs + static_cast<size_t>(c1) * a.V.row + (32u * s + 8u * g) * 2u);
        }
    };
    if (it.nsteps) load_kv(st);
    // BIAS: the step's positions (kept for the GBias stores) and biases. The next step's positions
    // are requested before the K rows are staged, its values once this step's weights are formed (the
    // registers of this step's values take them: a second set spills at 128 / 128), so they are in
    // flight under the second product
    const u32* bs = BIAS ? a.base + static_cast<size_t>(it.step0) * PANEL_ROWS : nullptr;
    const float* bias = BIAS ? a.bias + slice * a.biasStride : nullptr;
    float* gbias = BIAS && a.gbias ? a.gbias + slice * a.gbiasStride : nullptr;
    u32 pc[BIAS ? 8 : 1], pn[BIAS ? 8 : 1];
    float b[BIAS ? 8 : 1];
    if constexpr (BIAS) {
        if (it.nsteps) {
            bias_positions(a.pos, st->masks[r], bs[r], g, pc);
            bias_values(bias, pc, b);
        }
    }
    for (u32 step = 0; step < it.nsteps; ++step, ++st) {
        const u32 colv = st->cols[lane & 31u];  // lane x holds step column x & 31
        const u32 mask = st->masks[r];
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f}, g0 = {0.f, 0.f, 0.f, 0.f}, g1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            s0 = mfma32<DT>(k0[s], q[s], s0);
            s1 = mfma32<DT>(k1[s], q[s], s1);
        }
#pragma unroll
        for (int s = 0; s < VS; ++s) {
            g0 = mfma32<DT>(v0[s], go[s], g0);
            g1 = mfma32<DT>(v1[s], go[s], g1);
        }
        if (step + 1 < it.nsteps) load_kv(st + 1);
        if constexpr (BIAS) {
            bs += PANEL_ROWS;
            if (step + 1 < it.nsteps) bias_positions(a.pos, st[1].masks[r], bs[r], g, pn);
        }

        // the step's K rows into LDS: chunk x = 64 u + lane is 16 bytes of row x / CPR. The reads of
        // the step before are done first
        wave_lds_sync();
        {
            uint4 kk[KLOADS];
#pragma unroll
            for (int u = 0; u < KLOADS; ++u) {
                const u32 x = 64u * u + lane;
                const u32 col = __shfl(colv, static_cast<int>(x / CPR));
                kk[u] = load16(Ks + static_cast<size_t>(col) * a.K.row + (x % CPR) * 16u);
            }
#pragma unroll
            for (int u = 0; u < KLOADS; ++u) {
                const u32 x = 64u * u + lane;
                *reinterpret_cast<uint4*>(kl + (x / CPR) * KROW + (x % CPR) * 16u) = kk[u];
            }
        }

        float w, dp[8];
        if constexpr (BIAS) {
            float h[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                panel_weight<true>(s0[j], g0[j], lse, dl, a.scale, (mask >> panel_slot(g, j)) & 1u, w, dp[j], b[j], &h[j]);
                panel_weight<true>(s1[j], g1[j], lse, dl, a.scale, (mask >> panel_slot(g, 4 + j)) & 1u, w, dp[4 + j], b[4 + j],
                                   &h[4 + j]);
            }
            // GBias: one 4-byte store per set mask bit; every stored entry lies in one step of one item
            if (gbias) {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (pc[j] != NO_ENTRY) gbias[pc[j]] = h[j];
            }
            if (step + 1 < it.nsteps) {  // (the positions arrived under the K loads)
#pragma unroll
                for (int j = 0; j < 8; ++j) pc[j] = pn[j];
                bias_values(bias, pc, b);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                panel_weight(s0[j], g0[j], lse, dl, a.scale, (mask >> panel_slot(g, j)) & 1u, w, dp[j]);
                panel_weight(s1[j], g1[j], lse, dl, a.scale, (mask >> panel_slot(g, 4 + j)) & 1u, w, dp[4 + j]);
            }
        }
        const uint4 pb = pack8<DT>(dp);

        wave_lds_sync();
#pragma unroll
        for (int n = 0; n < KS; ++n) {
            uint4 even, odd;
            staged_pair<KROW>(kl, n, r, g, even, odd);
            acc[2 * n] = mfma32<DT>(even, pb, acc[2 * n]);
            acc[2 * n + 1] = mfma32<DT>(odd, pb, acc[2 * n + 1]);
        }
    }
    if (!live) return;
    if (BIAS && !a.Y0.ptr) return;  // (only GBias was asked for)
    float* o = it.part == PANEL_DIRECT
                   ? reinterpret_cast<float*>(attn_slice_base(a.Y0, bat, head) + static_cast<size_t>(row) * a.Y0.row)
                   : a.P0 + ((slice * a.partials + it.part) * PANEL_ROWS + r) * D;
    store_acc<KS>(o + 8u * g, acc);
}

template <int DT, int D, int DV, bool BIAS>
__global__ __launch_bounds__(PANEL_WAVES * 64) __attribute__((amdgpu_waves_per_eu(2)))
void k_attention_bwd_panels_cols(const BwdPanelArgs a) {
    constexpr int KS = D / 32;                  // k-steps of a score tile, and pairs of GK tiles
    constexpr int VS = DV / 32;                 // k-steps of a g tile, and pairs of GV tiles
    constexpr u32 QROW = staged_row_bytes(D);   // bytes between staged Q rows
    constexpr u32 GROW = staged_row_bytes(DV);  // bytes between staged GO rows (operand type)
    constexpr u32 QCPR = D / 8, GCPR = DV / 8;  // 16-byte chunks per staged row
    constexpr int QLOADS = D / 16, GLOADS = DV / 16;
    __shared__ __attribute__((aligned(16))) char stage[PANEL_WAVES][PANEL_STEP_COLS * (QROW + GROW)];

    const u32 lane = threadIdx.x & 63u;
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 itemId = blockIdx.x * PANEL_WAVES + wave;
    if (itemId >= a.nItems) return;
    const PanelItem it = a.items[itemId];
    const u32 head = blockIdx.y, bat = blockIdx.z;
    const size_t slice = static_cast<size_t>(bat) * a.heads + head;
    const char* Qs = attn_slice_base(a.Q, bat, head);
    const char* Ks = attn_slice_base(a.K, bat, head);
    const char* Vs = attn_slice_base(a.V, bat, head);
    const char* GOs = attn_slice_base(a.GO, bat, head);
    const float* const lses = a.lse + slice * a.M;
    const float* const deltas = a.delta + slice * a.M;
    char* ql = stage[wave];
    char* gl = ql + PANEL_STEP_COLS * QROW;

    const u32 c = lane & 15u, g = lane >> 4;
    const bool live = it.row0 + c < a.nDst;  // (a column of a short last panel is neither loaded nor stored)
    const u32 col = it.row0 + c;
    uint4 k[KS], v[VS];
#pragma unroll
    for (int s = 0; s < KS; ++s)
        k[s] = live ? load16(Ks + static_cast<size_t>(col) * a.K.row + (32u * s + 8u * g) * 2u) : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int s = 0; s < VS; ++s)
        v[s] = live ? load16(Vs + static_cast<size_t>(col) * a.V.row + (32u * s + 8u * g) * 2u) : make_uint4(0, 0, 0, 0);

    f32x4 accK[2 * KS], accV[2 * VS];
#pragma unroll
    for (int n = 0; n < 2 * KS; ++n) accK[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int n = 0; n < 2 * VS; ++n) accV[n] = f32x4{0.f, 0.f, 0.f, 0.f};

    const PanelStep* st = a.steps + it.step0;
    const u32* bs = BIAS ? a.base + static_cast<size_t>(it.step0) * PANEL_ROWS : nullptr;
    const float* bias = BIAS ? a.bias + slice * a.biasStride : nullptr;
    for (u32 step = 0; step < it.nsteps; ++step, ++st) {
        const u32 rowv = st->cols[lane & 31u];  // lane x holds step row x & 31 with its LSE and delta
        const u32 mask = st->masks[c];
        const float lsev = lses[rowv], dlv = deltas[rowv];
        // BIAS: the positions of the column's entries at the lane's step rows are requested before the
        // stage's loads and the values after them, so both rounds lie under the staging
        u32 pc[BIAS ? 8 : 1];
        float b[BIAS ? 8 : 1];
        if constexpr (BIAS) {
            bias_positions(a.pos, mask, bs[c], g, pc);
            bs += PANEL_ROWS;
        }

        // the step's Q rows and rounded GO rows into LDS; the reads of the step before are done first
        wave_lds_sync();
#pragma unroll
        for (int u0 = 0; u0 < QLOADS; u0 += 4) {  // (four chunks in flight: eight spill at 128 / 128)
            constexpr int QB = QLOADS < 4 ? QLOADS : 4;
            uint4 qq[QB];
#pragma unroll
            for (int u = 0; u < QB; ++u) {
                const u32 x = 64u * (u0 + u) + lane;
                const u32 row = __shfl(rowv, static_cast<int>(x / QCPR));
                qq[u] = load16(Qs + static_cast<size_t>(row) * a.Q.row + (x % QCPR) * 16u);
            }
#pragma unroll
            for (int u = 0; u < QB; ++u) {
                const u32 x = 64u * (u0 + u) + lane;
                *reinterpret_cast<uint4*>(ql + (x / QCPR) * QROW + (x % QCPR) * 16u) = qq[u];
            }
        }
#pragma unroll
        for (int u0 = 0; u0 < GLOADS; u0 += 4) {
            constexpr int GB = GLOADS < 4 ? GLOADS : 4;
            uint4 gg[GB];
#pragma unroll
            for (int u = 0; u < GB; ++u) {
                const u32 x = 64u * (u0 + u) + lane;
                const u32 row = __shfl(rowv, static_cast<int>(x / GCPR));
                gg[u] = load8_rounded<DT>(GOs + static_cast<size_t>(row) * a.GO.row + (x % GCPR) * 32u);
            }
#pragma unroll
            for (int u = 0; u < GB; ++u) {
                const u32 x = 64u * (u0 + u) + lane;
                *reinterpret_cast<uint4*>(gl + (x / GCPR) * GROW + (x % GCPR) * 16u) = gg[u];
            }
        }
        if constexpr (BIAS) bias_values(bias, pc, b);
        wave_lds_sync();

        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f}, g0 = {0.f, 0.f, 0.f, 0.f}, g1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            s0 = mfma32<DT>(load16(ql + c * QROW + (32u * s + 8u * g) * 2u), k[s], s0);
            s1 = mfma32<DT>(load16(ql + (16u + c) * QROW + (32u * s + 8u * g) * 2u), k[s], s1);
        }
#pragma unroll
        for (int s = 0; s < VS; ++s) {
            g0 = mfma32<DT>(load16(gl + c * GROW + (32u * s + 8u * g) * 2u), v[s], g0);
            g1 = mfma32<DT>(load16(gl + (16u + c) * GROW + (32u * s + 8u * g) * 2u), v[s], g1);
        }

        float w[8], dp[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r0 = static_cast<int>(4u * g + j), r1 = static_cast<int>(16u + 4u * g + j);
            float h;
            panel_weight<BIAS>(s0[j], g0[j], __shfl(lsev, r0), __shfl(dlv, r0), a.scale, (mask >> r0) & 1u, w[j], dp[j],
                               BIAS ? b[j] : 0.f, &h);
            panel_weight<BIAS>(s1[j], g1[j], __shfl(lsev, r1), __shfl(dlv, r1), a.scale, (mask >> r1) & 1u, w[4 + j], dp[4 + j],
                               BIAS ? b[BIAS ? 4 + j : 0] : 0.f, &h);
        }
        const uint4 wb = pack8<DT>(w), pb = pack8<DT>(dp);
        // (the scheduler otherwise hoists both products' 16 (VS + KS) word reads over the weights: spills
        // at 128 / 128)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int n = 0; n < VS; ++n) {
            uint4 even, odd;
            staged_pair<GROW>(gl, n, c, g, even, odd);
            accV[2 * n] = mfma32<DT>(even, wb, accV[2 * n]);
            accV[2 * n + 1] = mfma32<DT>(odd, wb, accV[2 * n + 1]);
        }
#pragma unroll
        for (int n = 0; n < KS; ++n) {
            uint4 even, odd;
            staged_pair<QROW>(ql, n, c, g, even, odd);
            accK[2 * n] = mfma32<DT>(even, pb, accK[2 * n]);
            accK[2 * n + 1] = mfma32<DT>(odd, pb, accK[2 * n + 1]);
        }
    }
    if (!live) return;
    const bool direct = it.part == PANEL_DIRECT;
    const size_t slot = (slice * a.partials + (direct ? 0u : it.part)) * PANEL_ROWS + c;
    if (a.Y0.ptr) {
        float* o = direct ? reinterpret_cast<float*>(attn_slice_base(a.Y0, bat, head) + static_cast<size_t>(col) * a.Y0.row)
                          : a.P0 + slot * D;
        store_acc<KS>(o + 8u * g, accK);
    }
    if (a.Y1.ptr) {
        float* o = direct ? reinterpret_cast<float*>(attn_slice_base(a.Y1, bat, head) + static_cast<size_t>(col) * a.Y1.row)
                          : a.P1 + slot * DV;
        store_acc<VS>(o + 8u * g, accV);
    }
}

// a split panel's destinations: the partial slots added in item order, plain sums; one thread per
// destination and four columns of Y0 (W0 columns, or none: Y0 null) followed by Y1 (W1, or none)
__global__ __launch_bounds__(256) void k_attention_bwd_panels_reduce(const BwdPanelArgs a, const PanelRed* reds, u32 nReds,
                                                                     u32 W0, u32 W1) {
#pragma clang fp contract(off)
    const u32 head = blockIdx.y, bat = blockIdx.z;
    const size_t slice = static_cast<size_t>(bat) * a.heads + head;
    const u32 q0 = a.Y0.ptr ? W0 / 4u : 0u, q1 = a.Y1.ptr ? W1 / 4u : 0u, q4 = q0 + q1;
    const size_t t = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
    if (t >= static_cast<size_t>(nReds) * PANEL_ROWS * q4) return;
    const PanelRed rd = reds[t / (PANEL_ROWS * q4)];
    const u32 r = static_cast<u32>(t / q4) % PANEL_ROWS;
    u32 q = static_cast<u32>(t % q4);
    if (rd.row0 + r >= a.nDst) return;
    const u32 dst = a.rows ? a.rows[rd.row0 + r] : rd.row0 + r;
    const bool second = q >= q0;
    if (second) q -= q0;
    const u32 W = second ? W1 : W0;
    const AttnOpBytes& Y = second ? a.Y1 : a.Y0;
    const float* P = (second ? a.P1 : a.P0) + ((slice * a.partials + rd.part0) * PANEL_ROWS + r) * W;
    const float4* p = reinterpret_cast<const float4*>(P) + q;  // partials are 16 rows of W apart
    float4 s = p[0];
    for (u32 i = 1; i < rd.nparts; ++i) {
        const float4 x = p[static_cast<size_t>(i) * PANEL_ROWS * (W / 4u)];
        s.x += x.x;
        s.y += x.y;
        s.z += x.z;
        s.w += x.w;
    }
    reinterpret_cast<float4*>(attn_slice_base(Y, bat, head) + static_cast<size_t>(dst) * Y.row)[q] = s;
}

using BwdPanelFn = void (*)(const BwdPanelArgs);

template <int DT, int D, bool BIAS>
BwdPanelFn pick_dv(bool rows, u32 Dv) {
    switch (Dv) {
        case 32: return rows ? k_attention_bwd_panels_rows<DT, D, 32, BIAS> : k_attention_bwd_panels_cols<DT, D, 32, BIAS>;
        case 64: return rows ? k_attention_bwd_panels_rows<DT, D, 64, BIAS> : k_attention_bwd_panels_cols<DT, D, 64, BIAS>;
        case 128: return rows ? k_attention_bwd_panels_rows<DT, D, 128, BIAS> : k_attention_bwd_panels_cols<DT, D, 128, BIAS>;
        default: return nullptr;
    }
}

template <int DT, bool BIAS>
BwdPanelFn pick_d(bool rows, u32 D, u32 Dv) {
    switch (D) {
        case 32: return pick_dv<DT, 32, BIAS>(rows, Dv);
        case 64: return pick_dv<DT, 64, BIAS>(rows, Dv);
        case 128: return pick_dv<DT, 128, BIAS>(rows, Dv);
        default: return nullptr;
    }
}

template <bool BIAS>
BwdPanelFn pick_kernel(bool rows, u32 D, u32 Dv, int dtype) {
    return dtype == BSMR_F16 ? pick_d<BSMR_F16, BIAS>(rows, D, Dv) : pick_d<BSMR_BF16, BIAS>(rows, D, Dv);
}

size_t bwdp_row_floats(const Plan& p, u32 D, u32 slices) {
    return attn_sat_mul(attn_sat_mul(slices, p.panel_rows.partials, PANEL_ROWS), D);
}
size_t bwdp_col_floats(const Plan& p, u32 D, u32 Dv, u32 slices) {
    return attn_sat_mul(attn_sat_mul(slices, p.panel_cols.partials, PANEL_ROWS), static_cast<size_t>(D) + Dv);
}

bool bwdp_ready(const Plan& p, u32 D, u32 Dv, u32 slices) {
    const Plan::AttentionBwdPanelsState& B = p.attention_bwd_panels;
    return p.panel_cols.built && p.panel_rows.built && B.delta.size() >= attn_sat_mul(slices, p.M) &&
           B.rowScratch.size() >= bwdp_row_floats(p, D, slices) && B.colScratch.size() >= bwdp_col_floats(p, D, Dv, slices);
}

// the rows' lists (the forward's, built here when no forward has), the columns' lists (once) and
// delta and the per-slice scratches for (D, Dv, slices): they grow and never shrink; layout_mu
// held. Synchronous on the plan's stream.
int build_bwdp(const Plan& p, u32 D, u32 Dv, u32 slices, const char* who) {
    Plan::AttentionBwdPanelsState& B = p.attention_bwd_panels;
    BSMR_CHECK(attn_panels_build_lists(p, who));
    BSMR_CHECK(attn_bwd_panels_build_col_lists(p, who));
    BSMR_CHECK(B.delta.grow(attn_sat_mul(slices, p.M)));
    BSMR_CHECK(B.rowScratch.grow(bwdp_row_floats(p, D, slices)));
    BSMR_CHECK(B.colScratch.grow(bwdp_col_floats(p, D, Dv, slices)));
    return BSMR_OK;
}

struct BwdPanelOperands {
    const bsmr_attention_operand *Q, *K, *V, *O, *GO, *GQ, *GK, *GV;  // the last three may be null, not all
};

// the per-entry bias of a biased backward and its gradient (null: not asked for), nnz fp32 values at
// CSR positions per slice, strides in elements (bias: 0 is one for all slices)
struct BwdPanelBias {
    const float* bias;
    u64 biasStride;
    float* gbias;
    u64 gbiasStride;
};

// the biased backward also needs both sides' entry positions (the one copy in Plan::spmm_panels,
// spmm_panels_build_positions; no scratch of the panel SpMM)
bool bwdp_bias_ready(const Plan& p, u32 D, u32 Dv, u32 slices) {
    return bwdp_ready(p, D, Dv, slices) && p.spmm_panels[0].built && p.spmm_panels[1].built;
}

int build_bwdp_bias(const Plan& p, u32 D, u32 Dv, u32 slices, const char* who) {
    BSMR_CHECK(build_bwdp(p, D, Dv, slices, who));
    BSMR_CHECK(spmm_panels_build_positions(p, 1, who));
    return spmm_panels_build_positions(p, 2, who);
}

// the launches of bsmr_attention_backward_panels, its heads form and their biased forms (`bias`),
// arguments already validated
int bwdp_launch(const char* who, const char* prep, const bsmr_plan* plan, u32 batches, u32 heads, const BwdPanelOperands& x,
                const float* dLse, u32 D, u32 Dv, int dtype, float scale, void* stream, const BwdPanelBias* bias = nullptr) {
    const Plan& p = plan->p;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const u32 slices = batches * heads;  // (both at most 65535)
    BwdPanelArgs r{}, cs{};
    const PanelRed *rreds = nullptr, *creds = nullptr;
    u32 rowReds = 0, colReds = 0;
    float* delta = nullptr;
    {
        std::lock_guard<std::mutex> g(p.layout_mu);
        BSMR_CHECK(panel_build_missing(
            LaunchSite{s, who, prep, D, dtype},
            [&] { return bias ? bwdp_bias_ready(p, D, Dv, slices) : bwdp_ready(p, D, Dv, slices); },
            [&] {
                return std::string("the panel backward's lists") + (bias ? ", the entry positions" : "") +
                       " (or their scratch for D = " + std::to_string(D) + ", Dv = " + std::to_string(Dv) +
                       panel_slices_clause(slices) + ")";
            },
            [&] { return bias ? build_bwdp_bias(p, D, Dv, slices, prep) : build_bwdp(p, D, Dv, slices, prep); }));
        const Plan::PanelListState &R = p.panel_rows, &C = p.panel_cols;
        const Plan::AttentionBwdPanelsState& B = p.attention_bwd_panels;
        r.items = R.items.data();
        r.steps = R.steps.data();
        r.rows = R.rows.data();
        r.nItems = R.nItems;
        r.partials = R.partials;
        r.P0 = B.rowScratch.data();
        rreds = R.reds.data();
        rowReds = R.nReds;
        cs.items = C.items.data();
        cs.steps = C.steps.data();
        cs.nItems = C.nItems;
        cs.partials = C.partials;
        cs.P0 = B.colScratch.data();
        creds = C.reds.data();
        colReds = C.nReds;
        delta = B.delta.data();
        if (bias) {
            r.base = p.spmm_panels[0].base.data();
            r.pos = p.spmm_panels[0].pos.data();
            cs.base = p.spmm_panels[1].base.data();
            cs.pos = p.spmm_panels[1].pos.data();
        }
    }
    if (bias) {
        r.bias = cs.bias = bias->bias;
        r.biasStride = cs.biasStride = bias->biasStride;
        r.gbias = bias->gbias;
        r.gbiasStride = bias->gbiasStride;
    }
    cs.P1 = cs.P0 ? cs.P0 + static_cast<size_t>(slices) * cs.partials * PANEL_ROWS * D : nullptr;
    r.Q = cs.Q = attn_op_bytes(x.Q, batches, heads, p.M, 2u);
    r.K = cs.K = attn_op_bytes(x.K, batches, heads, p.N, 2u);
    r.V = cs.V = attn_op_bytes(x.V, batches, heads, p.N, 2u);
    r.GO = cs.GO = attn_op_bytes(x.GO, batches, heads, p.M, 4u);
    r.lse = cs.lse = dLse;
    r.delta = cs.delta = delta;
    r.heads = cs.heads = heads;
    r.M = cs.M = p.M;
    r.nDst = p.M;
    cs.nDst = p.N;
    r.scale = cs.scale = scale;
    r.Y0 = attn_op_bytes(x.GQ, batches, heads, p.M, 4u);
    cs.Y0 = attn_op_bytes(x.GK, batches, heads, p.N, 4u);
    cs.Y1 = attn_op_bytes(x.GV, batches, heads, p.N, 4u);

    BSMR_CHECK(attn_bwd_launch_delta(r.GO, attn_op_bytes(x.O, batches, heads, p.M, 4u), delta, batches, heads, p.M, D, Dv, 2u, s));
    auto side = [&](const BwdPanelArgs& a, bool rows, const PanelRed* reds, u32 nReds, u32 q4) {
        const dim3 outer(1, heads, batches);
        return panel_launch(s, bias ? pick_kernel<true>(rows, D, Dv, dtype) : pick_kernel<false>(rows, D, Dv, dtype), a, a.nItems,
                            outer, k_attention_bwd_panels_reduce, reds, nReds, q4, outer, D, Dv);
    };
    // (the rows side also runs for GBias alone: it then stores no GQ and has nothing to reduce)
    if (x.GQ || (bias && bias->gbias)) BSMR_CHECK(side(r, true, rreds, x.GQ ? rowReds : 0u, D / 4u));
    if (x.GK || x.GV) BSMR_CHECK(side(cs, false, creds, colReds, (x.GK ? D / 4u : 0u) + (x.GV ? Dv / 4u : 0u)));
    return BSMR_OK;
}

}  // namespace

// the column panels' lists (once): attention_panel_lists on the transposed pattern, M and N in each
// other's role and no order, so a column panel is 16 consecutive columns. The panel SpMM's columns
// side (spmm_panels.hip) runs over these very lists and builds them through this when no backward has
int attn_bwd_panels_build_col_lists(const Plan& p, const char* who) {
    if (p.panel_cols.built) return BSMR_OK;
    const hipStream_t s = p.stream;
    std::vector<u32> hrp, hci, trp, tci;
    BSMR_CHECK(p.rowptr.download(hrp, s));
    BSMR_CHECK(p.colidx.download(hci, s));
    PanelLists L;
    std::string err;
    if (attention_pattern_transpose(p.M, p.N, hrp.data(), hci.data(), trp, tci, err)) {
        set_error(std::string(who) + ": " + err);
        return BSMR_ERR_INVALID;
    }
    const int st = attention_panel_lists(p.N, p.M, trp.data(), tci.data(), nullptr, 0, L, err);
    L.rows.clear();  // (the identity: a column is its position, and the kernels take a null order)
    return panel_lists_upload(p, p.panel_cols, st, err, L, who);
}

}  // namespace bsmr

using namespace bsmr;

extern "C" int bsmr_attention_backward_panels(const bsmr_plan* plan, const void* dQ, const void* dK, const void* dV,
                                              const float* dO, const float* dGO, const float* dLse, uint32_t D, uint32_t Dv,
                                              int dtype, float scale, float* dGQ, float* dGK, float* dGV, void* stream) {
    const char* who = "bsmr_attention_backward_panels";
    if (!plan) {
        set_error("bsmr_attention_backward_panels: null plan");
        return BSMR_ERR_INVALID;
    }
    if (!dQ || !dK || !dV || !dO || !dGO || !dLse) {
        set_error("bsmr_attention_backward_panels: null device pointer");
        return BSMR_ERR_INVALID;
    }
    if (!dGQ && !dGK && !dGV) {
        set_error("bsmr_attention_backward_panels: dGQ, dGK and dGV are all null: nothing to compute");
        return BSMR_ERR_INVALID;
    }
    if (!attn_aligned16(dQ) || !attn_aligned16(dK) || !attn_aligned16(dV) || !attn_aligned16(dO) ||
        !attn_aligned16(dGO) || !attn_aligned16(dGQ) || !attn_aligned16(dGK) || !attn_aligned16(dGV) ||
        (reinterpret_cast<uintptr_t>(dLse) & 3u)) {
        set_error("bsmr_attention_backward_panels: dQ, dK, dV, dO, dGO, dGQ, dGK and dGV must be 16-byte aligned");
        return BSMR_ERR_INVALID;
    }
    float c;
    BSMR_CHECK(attn_validate_scale(who, scale, &c));
    BSMR_CHECK(panel_validate_dims(who, D, Dv, dtype, false));
    const Plan& p = plan->p;
    const bsmr_attention_operand q = attention_dense_operand(dQ, 1, p.M, D), k = attention_dense_operand(dK, 1, p.N, D),
                                 v = attention_dense_operand(dV, 1, p.N, Dv), o = attention_dense_operand(dO, 1, p.M, Dv),
                                 go = attention_dense_operand(dGO, 1, p.M, Dv), gq = attention_dense_operand(dGQ, 1, p.M, D),
                                 gk = attention_dense_operand(dGK, 1, p.N, D), gv = attention_dense_operand(dGV, 1, p.N, Dv);
    const BwdPanelOperands x{&q, &k, &v, &o, &go, dGQ ? &gq : nullptr, dGK ? &gk : nullptr, dGV ? &gv : nullptr};
    return bwdp_launch(who, "bsmr_plan_prepare_attention_backward_panels", plan, 1, 1, x, dLse, D, Dv, dtype, scale, stream);
}

extern "C" int bsmr_attention_backward_panels_heads(const bsmr_plan* plan, uint32_t batches, uint32_t heads,
                                                    const bsmr_attention_operand* Q, const bsmr_attention_operand* K,
                                                    const bsmr_attention_operand* V, const bsmr_attention_operand* O,
                                                    const bsmr_attention_operand* GO, const float* dLse, uint32_t D,
                                                    uint32_t Dv, int dtype, float scale, const bsmr_attention_operand* GQ,
                                                    const bsmr_attention_operand* GK, const bsmr_attention_operand* GV,
                                                    void* stream) {
    const char* who = "bsmr_attention_backward_panels_heads";
    if (!plan) {
        set_error("bsmr_attention_backward_panels_heads: null plan");
        return BSMR_ERR_INVALID;
    }
    if (!dLse || (reinterpret_cast<uintptr_t>(dLse) & 3u)) {
        set_error("bsmr_attention_backward_panels_heads: dLse must be non-null and 4-byte aligned");
        return BSMR_ERR_INVALID;
    }
    if (!GQ && !GK && !GV) {
        set_error("bsmr_attention_backward_panels_heads: GQ, GK and GV are all null: nothing to compute");
        return BSMR_ERR_INVALID;
    }
    float c;
    BSMR_CHECK(attn_validate_scale(who, scale, &c));
    BSMR_CHECK(panel_validate_dims(who, D, Dv, dtype, false));
    const Plan& p = plan->p;
    BSMR_CHECK(attn_check_operand(who, "Q", Q, batches, heads, p.M, D, 2u, false));
    BSMR_CHECK(attn_check_operand(who, "K", K, batches, heads, p.N, D, 2u, false));
    BSMR_CHECK(attn_check_operand(who, "V", V, batches, heads, p.N, Dv, 2u, false));
    BSMR_CHECK(attn_check_operand(who, "O", O, batches, heads, p.M, Dv, 4u, false));
    BSMR_CHECK(attn_check_operand(who, "GO", GO, batches, heads, p.M, Dv, 4u, false));
    if (GQ) BSMR_CHECK(attn_check_operand(who, "GQ", GQ, batches, heads, p.M, D, 4u, true));
    if (GK) BSMR_CHECK(attn_check_operand(who, "GK", GK, batches, heads, p.N, D, 4u, true));
    if (GV) BSMR_CHECK(attn_check_operand(who, "GV", GV, batches, heads, p.N, Dv, 4u, true));
    const BwdPanelOperands x{Q, K, V, O, GO, GQ, GK, GV};
    return bwdp_launch(who, "bsmr_plan_prepare_attention_backward_panels_heads", plan, batches, heads, x, dLse, D, Dv, dtype,
                       scale, stream);
}

extern "C" int bsmr_plan_prepare_attention_backward_panels_heads(const bsmr_plan* plan, uint32_t D, uint32_t Dv,
                                                                 uint32_t slices) {
    const char* who = "bsmr_plan_prepare_attention_backward_panels_heads";
    BSMR_CHECK(panel_prepare_args(who, plan, D, Dv, slices, false));
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return build_bwdp(plan->p, D, Dv, slices, who);
}

extern "C" int bsmr_plan_prepare_attention_backward_panels(const bsmr_plan* plan, uint32_t D, uint32_t Dv) {
    const char* who = "bsmr_plan_prepare_attention_backward_panels";
    BSMR_CHECK(panel_prepare_args(who, plan, D, Dv, 1, false));
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return build_bwdp(plan->p, D, Dv, 1, who);
}

extern "C" int bsmr_plan_attention_backward_panels_heads_prepared(const bsmr_plan* plan, uint32_t D, uint32_t Dv,
                                                                  uint32_t slices) {
    if (panel_prepare_args("bsmr_plan_attention_backward_panels_heads_prepared", plan, D, Dv, slices, false) != BSMR_OK) return 0;
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return bwdp_ready(plan->p, D, Dv, slices) ? 1 : 0;
}

extern "C" int bsmr_plan_attention_backward_panels_prepared(const bsmr_plan* plan, uint32_t D, uint32_t Dv) {
    return bsmr_plan_attention_backward_panels_heads_prepared(plan, D, Dv, 1);
}

extern "C" int bsmr_plan_attention_backward_panels_stats(const bsmr_plan* plan, bsmr_attention_backward_panels_stats* out) {
    if (!plan || !out) {
        set_error("bsmr_plan_attention_backward_panels_stats: null argument");
        return BSMR_ERR_INVALID;
    }
    const Plan& p = plan->p;
    std::lock_guard<std::mutex> g(p.layout_mu);
    const Plan::AttentionBwdPanelsState& B = p.attention_bwd_panels;
    *out = bsmr_attention_backward_panels_stats{};
    if (p.panel_cols.built && p.panel_rows.built) {
        panel_list_stats(p.panel_rows, p.nnz, out->row_panels, out->row_items, out->row_steps, out->row_split_panels,
                         out->row_partials, out->row_fill_permille);
        panel_list_stats(p.panel_cols, p.nnz, out->col_panels, out->col_items, out->col_steps, out->col_split_panels,
                         out->col_partials, out->col_fill_permille);
        out->row_scratch_bytes = B.rowScratch.size() * sizeof(float);
        out->col_scratch_bytes = B.colScratch.size() * sizeof(float);
        out->delta_bytes = B.delta.size() * sizeof(float);
    }
    return BSMR_OK;
}

// ---- the biased forms (x = fl(p scale) + bias; attention_panels_bias.hip is the forward) ----

// what the biased entry points check beyond the unbiased ones: dBias, dGBias and their strides
static int bwd_bias_check(const char* who, const bsmr_plan* plan, const float* dBias, u64 biasStride, const float* dGBias,
                          u64 gbiasStride) {
    BSMR_CHECK(attn_panels_check_bias(who, plan, dBias, biasStride));
    if (reinterpret_cast<uintptr_t>(dGBias) & 3u) {
        set_error(std::string(who) + ": dGBias must be 4-byte aligned");
        return BSMR_ERR_INVALID;
    }
    if (dGBias && gbiasStride < plan->p.nnz) {
        set_error(std::string(who) + ": gbias_slice_stride must be at least nnz (a shared bias gets one gradient per slice)");
        return BSMR_ERR_INVALID;
    }
    return BSMR_OK;
}

extern "C" int bsmr_attention_backward_panels_bias(const bsmr_plan* plan, const void* dQ, const void* dK, const void* dV,
                                                   const float* dBias, const float* dO, const float* dGO, const float* dLse,
                                                   uint32_t D, uint32_t Dv, int dtype, float scale, float* dGQ, float* dGK,
                                                   float* dGV, float* dGBias, void* stream) {
    const char* who = "bsmr_attention_backward_panels_bias";
    if (!plan) {
        set_error(std::string(who) + ": null plan");
        return BSMR_ERR_INVALID;
    }
    if (!dQ || !dK || !dV || !dO || !dGO || !dLse) {
        set_error(std::string(who) + ": null device pointer");
        return BSMR_ERR_INVALID;
    }
    if (!dGQ && !dGK && !dGV && !dGBias) {
        set_error(std::string(who) + ": dGQ, dGK, dGV and dGBias are all null: nothing to compute");
        return BSMR_ERR_INVALID;
    }
    if (!attn_aligned16(dQ) || !attn_aligned16(dK) || !attn_aligned16(dV) || !attn_aligned16(dO) ||
        !attn_aligned16(dGO) || !attn_aligned16(dGQ) || !attn_aligned16(dGK) || !attn_aligned16(dGV) ||
        (reinterpret_cast<uintptr_t>(dLse) & 3u)) {
        set_error(std::string(who) + ": dQ, dK, dV, dO, dGO, dGQ, dGK and dGV must be 16-byte aligned");
        return BSMR_ERR_INVALID;
    }
    const Plan& p = plan->p;
    BSMR_CHECK(bwd_bias_check(who, plan, dBias, 0, dGBias, p.nnz));
    float c;
    BSMR_CHECK(attn_validate_scale(who, scale, &c));
    BSMR_CHECK(panel_validate_dims(who, D, Dv, dtype, false));
    const bsmr_attention_operand q = attention_dense_operand(dQ, 1, p.M, D), k = attention_dense_operand(dK, 1, p.N, D),
                                 v = attention_dense_operand(dV, 1, p.N, Dv), o = attention_dense_operand(dO, 1, p.M, Dv),
                                 go = attention_dense_operand(dGO, 1, p.M, Dv), gq = attention_dense_operand(dGQ, 1, p.M, D),
                                 gk = attention_dense_operand(dGK, 1, p.N, D), gv = attention_dense_operand(dGV, 1, p.N, Dv);
    const BwdPanelOperands x{&q, &k, &v, &o, &go, dGQ ? &gq : nullptr, dGK ? &gk : nullptr, dGV ? &gv : nullptr};
    const BwdPanelBias b{dBias, 0, dGBias, p.nnz};
    return bwdp_launch(who, "bsmr_plan_prepare_attention_backward_panels_bias", plan, 1, 1, x, dLse, D, Dv, dtype, scale, stream,
                       &b);
}

extern "C" int bsmr_attention_backward_panels_bias_heads(
    const bsmr_plan* plan, uint32_t batches, uint32_t heads, const bsmr_attention_operand* Q, const bsmr_attention_operand* K,
    const bsmr_attention_operand* V, const float* dBias, uint64_t bias_slice_stride, const bsmr_attention_operand* O,
    const bsmr_attention_operand* GO, const float* dLse, uint32_t D, uint32_t Dv, int dtype, float scale,
    const bsmr_attention_operand* GQ, const bsmr_attention_operand* GK, const bsmr_attention_operand* GV, float* dGBias,
    uint64_t gbias_slice_stride, void* stream) {
    const char* who = "bsmr_attention_backward_panels_bias_heads";
    if (!plan) {
        set_error(std::string(who) + ": null plan");
        return BSMR_ERR_INVALID;
    }
    if (!dLse || (reinterpret_cast<uintptr_t>(dLse) & 3u)) {
        set_error(std::string(who) + ": dLse must be non-null and 4-byte aligned");
        return BSMR_ERR_INVALID;
    }
    if (!GQ && !GK && !GV && !dGBias) {
        set_error(std::string(who) + ": GQ, GK, GV and dGBias are all null: nothing to compute");
        return BSMR_ERR_INVALID;
    }
    BSMR_CHECK(bwd_bias_check(who, plan, dBias, bias_slice_stride, dGBias, gbias_slice_stride));
    float c;
    BSMR_CHECK(attn_validate_scale(who, scale, &c));
    BSMR_CHECK(panel_validate_dims(who, D, Dv, dtype, false));
    const Plan& p = plan->p;
    BSMR_CHECK(attn_check_operand(who, "Q", Q, batches, heads, p.M, D, 2u, false));
    BSMR_CHECK(attn_check_operand(who, "K", K, batches, heads, p.N, D, 2u, false));
    BSMR_CHECK(attn_check_operand(who, "V", V, batches, heads, p.N, Dv, 2u, false));
    BSMR_CHECK(attn_check_operand(who, "O", O, batches, heads, p.M, Dv, 4u, false));
    BSMR_CHECK(attn_check_operand(who, "GO", GO, batches, heads, p.M, Dv, 4u, false));
    if (GQ) BSMR_CHECK(attn_check_operand(who, "GQ", GQ, batches, heads, p.M, D, 4u, true));
    if (GK) BSMR_CHECK(attn_check_operand(who, "GK", GK, batches, heads, p.N, D, 4u, true));
    if (GV) BSMR_CHECK(attn_check_operand(who, "GV", GV, batches, heads, p.N, Dv, 4u, true));
    const BwdPanelOperands x{Q, K, V, O, GO, GQ, GK, GV};
    const BwdPanelBias b{dBias, bias_slice_stride, dGBias, gbias_slice_stride};
    return bwdp_launch(who, "bsmr_plan_prepare_attention_backward_panels_bias_heads", plan, batches, heads, x, dLse, D, Dv, dtype,
                       scale, stream, &b);
}

extern "C" int bsmr_plan_prepare_attention_backward_panels_bias_heads(const bsmr_plan* plan, uint32_t D, uint32_t Dv,
                                                                      uint32_t slices) {
    const char* who = "bsmr_plan_prepare_attention_backward_panels_bias_heads";
    BSMR_CHECK(panel_prepare_args(who, plan, D, Dv, slices, false));
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return build_bwdp_bias(plan->p, D, Dv, slices, who);
}

extern "C" int bsmr_plan_prepare_attention_backward_panels_bias(const bsmr_plan* plan, uint32_t D, uint32_t Dv) {
    const char* who = "bsmr_plan_prepare_attention_backward_panels_bias";
    BSMR_CHECK(panel_prepare_args(who, plan, D, Dv, 1, false));
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return build_bwdp_bias(plan->p, D, Dv, 1, who);
}

extern "C" int bsmr_plan_attention_backward_panels_bias_heads_prepared(const bsmr_plan* plan, uint32_t D, uint32_t Dv,
                                                                       uint32_t slices) {
    if (panel_prepare_args("bsmr_plan_attention_backward_panels_bias_heads_prepared", plan, D, Dv, slices, false) != BSMR_OK)
        return 0;
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return bwdp_bias_ready(plan->p, D, Dv, slices) ? 1 : 0;
}

extern "C" int bsmr_plan_attention_backward_panels_bias_prepared(const bsmr_plan* plan, uint32_t D, uint32_t Dv) {
    return bsmr_plan_attention_backward_panels_bias_heads_prepared(plan, D, Dv, 1);
}
