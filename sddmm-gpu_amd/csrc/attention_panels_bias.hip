// attention_panels_bias.hip — the panel forward of attention_panels.hip with an additive bias per
// stored entry (bsmr_attention_panels_bias; fp16 / bf16 operands, bias nnz fp32 values at CSR
// positions, the layout of bsmr_spmm's V and bsmr_sddmm's P):
//
//   x_e = fl(p_e scale) + bias_e,  W = softmax over row i of x,  O[i,:] = sum_e W_e V[j_e,:],
//   LSE_i = log sum_e exp(x_e)
//
// with p_e = dot(Q[i,:], K[j_e,:]) out of the MFMA, the product and the sum each rounded on their own
// (no fma). Lists, items, the four waves of a workgroup, both transposed products, the V stage, the
// partials and k_attention_panels_reduce are attention_panels.hip's. What is new is the gather of the
// bias into the registers that hold a row's scores, and the softmax running in x's units.
// With r = l & 15 and g = l >> 4:
//   gather   lane (r, g) owns row r's scores at the step slots panel_slot(g, j), j = 0 .. 7
//            (panel_mfma.hpp). The entry of slot c lies at pos[base[16 s + r] + popcount(mask_r below
//            c)] of the bias (spmm_panels.hpp; the rows side's positions, Plan::spmm_panels[0]): two
//            dependent rounds of eight 4-byte loads, each predicated on the lane's mask bit, so a
//            clear bit (a padding slot, a column of another row, a row past the panel's end) issues
//            neither;
//   schedule k_spmm_panels': the positions of step s + 1 are requested after step s's score MFMAs and
//            the request of step s + 1's K rows, before step s's V rows are staged; the values right
//            after the stage's stores, when the positions have arrived under the V loads. Both rounds
//            are in flight under the step's softmax and its second product, and the values wait in
//            eight registers until step s + 1 forms x;
//   softmax  x = fl(p scale) + bias where the mask bit is set, -inf where it is clear, whatever p
//            was; m' = max(m, max x), f = 2^((m - m') log2e), t = 2^((x - m') log2e), shift_of and
//            inverse_of as before, LSE = m + log l. PanelArgs carries c = log2(e) rounded once and
//            scale = 1 for this form, so a split panel's (m, l, acc) go through the one reduce.
//
// Conventions: attention_panels.hip's, and: bias = -inf removes the entry (t = 0); a row whose
// entries are all -inf is an empty row (m = -inf, l = 0: O = 0, LSE = -inf, no NaN); a NaN or +inf
// bias makes exactly its own row NaN (t is the lane's B operand: column r of the product), like a
// NaN score.
//
// Resources: the 16-bit form's LDS; 24 registers more at the peak (eight positions, eight values in
// flight, eight values of the step). D, Dv in {32, 64, 128}: the 256 forms have no room for them
// (the unbiased (256, 256) form sits at 252 of 256) and are not built.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "attention_common.hpp"
#include "attention_layout.hpp"
#include "attention_panels.hpp"
#include "attention_panels_args.hpp"
#include "panel_host.hpp"
#include "panel_mfma.hpp"
#include "plan.hpp"
#include "seg_walk.hpp"  // exp2_hw

namespace bsmr {
namespace {

constexpr u32 NO_ENTRY = 0xFFFFFFFFu;  // the position of a slot whose mask bit is clear

// x of a stored entry: the product and the sum each rounded on their own
__device__ __forceinline__ float biased_score(float p, float scale, float b) {
#pragma clang fp contract(off)
    const float ps = p * scale;
    return ps + b;
}

template <int DT, int D, int DV>
__global__ __launch_bounds__(PANEL_WAVES * 64) __attribute__((amdgpu_waves_per_eu(2)))
void k_attention_panels_bias(const PanelArgs a) {
    constexpr int KS = D / 32;                  // k-steps of a score tile
    constexpr int NP = DV / 32;                 // pairs of output tiles
    constexpr u32 VROW = staged_row_bytes(DV);  // bytes between staged V rows
    constexpr u32 CPR = DV / 8;                 // 16-byte chunks per V row
    constexpr int VLOADS = DV / 16;             // chunks per lane and step (32 rows)
    constexpr int VBATCH = VLOADS < 8 ? VLOADS : 8;
    __shared__ __attribute__((aligned(16))) char vstage[PANEL_WAVES][PANEL_STEP_COLS * VROW];

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
    char* Os = attn_slice_base(a.O, bat, head);
    const float* bias = a.bias + slice * a.biasStride;
    char* vl = vstage[wave];

    const u32 r = lane & 15u, g = lane >> 4;
    const bool live = it.row0 + r < a.M;  // (a row of a short last panel is neither loaded nor stored)
    const u32 row = live ? a.rows[it.row0 + r] : 0u;
    uint4 q[KS];
    panel_row_operand(q, Qs + static_cast<size_t>(row) * a.Q.row, live, g);

    float m = -INFINITY, l = 0.f;
    f32x4 acc[2 * NP];
#pragma unroll
    for (int n = 0; n < 2 * NP; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

    const PanelStep* st = a.steps + it.step0;
    const u32* bs = a.base + static_cast<size_t>(it.step0) * PANEL_ROWS;
    uint4 k0[KS], k1[KS];
    auto load_k = [&](const PanelStep* sp) {
        const u32 c0 = sp->cols[r], c1 = sp->cols[16u + r];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            k0[s] = load16(Ks + static_cast<size_t>(c0) * a.K.row + (32u * s + 8u * g) * 2u);
            k1[s] = load16(Ks + static_cast<size_t>(c1) * a.K.row + (32u * s + 8u * g) * 2u);
        }
    };
    // a step's biases in two dependent rounds of loads, each predicated on the lane's mask bits
    auto load_pos = [&](const PanelStep* sp, const u32* bp, u32* p) {
        const u32 mask = sp->masks[r], b = bp[r];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const u32 c = panel_slot(g, j);
            p[j] = NO_ENTRY;
            if ((mask >> c) & 1u) p[j] = a.pos[b + __builtin_popcount(mask & ((1u << c) - 1u))];
        }
    };
    auto load_val = [&](const u32* p, float* w) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            w[j] = 0.f;
            if (p[j] != NO_ENTRY) w[j] = bias[p[j]];
        }
    };
    u32 pn[8];
    float b[8], bn[8];
    if (it.nsteps) {
        load_k(st);
        load_pos(st, bs, pn);
        load_val(pn, b);
    }
    for (u32 step = 0; step < it.nsteps; ++step, ++st, bs += PANEL_ROWS) {
        const u32 colv = st->cols[lane & 31u];  // lane x holds step column x & 31
        const u32 mask = st->masks[r];
        const bool more = step + 1 < it.nsteps;
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            s0 = mfma32<DT>(k0[s], q[s], s0);
            s1 = mfma32<DT>(k1[s], q[s], s1);
        }
        if (more) {
            load_k(st + 1);
            load_pos(st + 1, bs + PANEL_ROWS, pn);
        }

        // the step's V rows into LDS: chunk x = 64 u + lane is 16 bytes of row x / CPR. The reads
        // of the step before are done first
        wave_lds_sync();
#pragma unroll
        for (int u0 = 0; u0 < VLOADS; u0 += VBATCH) {
            uint4 v[VBATCH];
#pragma unroll
            for (int u = 0; u < VBATCH; ++u) {
                const u32 x = 64u * (u0 + u) + lane;
                const u32 col = __shfl(colv, static_cast<int>(x / CPR));
                v[u] = load16(Vs + static_cast<size_t>(col) * a.V.row + (x % CPR) * 16u);
            }
#pragma unroll
            for (int u = 0; u < VBATCH; ++u) {
                const u32 x = 64u * (u0 + u) + lane;
                *reinterpret_cast<uint4*>(vl + (x / CPR) * VROW + (x % CPR) * 16u) = v[u];
            }
        }
        if (more) load_val(pn, bn);  // (the positions arrived under the V loads)

        // x of the lane's row where it stores the column, the step's maximum and the weights
        float x[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            x[j] = (mask >> panel_slot(g, j)) & 1u ? biased_score(s0[j], a.xscale, b[j]) : -INFINITY;
            x[4 + j] = (mask >> panel_slot(g, 4 + j)) & 1u ? biased_score(s1[j], a.xscale, b[4 + j]) : -INFINITY;
        }
        float ms = x[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) ms = fmaxf(ms, x[j]);
        ms = fmaxf(ms, __shfl_xor(ms, 16));
        ms = fmaxf(ms, __shfl_xor(ms, 32));
        const float mn = fmaxf(m, ms);
        const float shift = shift_of(mn);
        const float f = exp2_hw((m - shift) * a.c);
        m = mn;
        float t[8], ts = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            t[j] = exp2_hw((x[j] - shift) * a.c);
            ts += t[j];
        }
        l = l * f + ts;
        const uint4 pb = pack8<DT>(t);
#pragma unroll
        for (int n = 0; n < 2 * NP; ++n) acc[n] *= f;

        wave_lds_sync();
#pragma unroll
        for (int n = 0; n < NP; ++n) {
            uint4 even, odd;
            staged_pair<VROW>(vl, n, r, g, even, odd);
            acc[2 * n] = mfma32<DT>(even, pb, acc[2 * n]);
            acc[2 * n + 1] = mfma32<DT>(odd, pb, acc[2 * n + 1]);
        }
        if (more) {
#pragma unroll
            for (int j = 0; j < 8; ++j) b[j] = bn[j];
        }
    }

    // the row's four lanes in g order: every lane of the row ends with the same sum
    const float lt = ((__shfl(l, static_cast<int>(r)) + __shfl(l, static_cast<int>(16u + r))) +
                      __shfl(l, static_cast<int>(32u + r))) + __shfl(l, static_cast<int>(48u + r));
    if (!live) return;
    // acc[2 n][j] and acc[2 n + 1][j] are columns 32 n + 8 g + 2 j and + 2 j + 1 of the row
    if (it.part == PANEL_DIRECT) {
        const float inv = inverse_of(lt);
        float* o = reinterpret_cast<float*>(Os + static_cast<size_t>(row) * a.O.row) + 8u * g;
#pragma unroll
        for (int n = 0; n < NP; ++n) {
            const f32x4 e = acc[2 * n], d = acc[2 * n + 1];
            *reinterpret_cast<float4*>(o + 32 * n) = make_float4(e[0] * inv, d[0] * inv, e[1] * inv, d[1] * inv);
            *reinterpret_cast<float4*>(o + 32 * n + 4) = make_float4(e[2] * inv, d[2] * inv, e[3] * inv, d[3] * inv);
        }
        if (g == 0 && a.lse) a.lse[slice * a.M + row] = m + logf(lt);  // (x's units: no scale)
    } else {
        const size_t slot = (slice * a.partials + it.part) * PANEL_ROWS + r;
        store_acc<NP>(a.pacc + slot * DV + 8u * g, acc);
        if (g == 0) {
            a.pml[2u * slot] = m;
            a.pml[2u * slot + 1u] = lt;
        }
    }
}

template <int DT, int D>
PanelFn pick_dv(u32 Dv) {
    switch (Dv) {
        case 32: return k_attention_panels_bias<DT, D, 32>;
        case 64: return k_attention_panels_bias<DT, D, 64>;
        case 128: return k_attention_panels_bias<DT, D, 128>;
        default: return nullptr;
    }
}

template <int DT>
PanelFn pick_d(u32 D, u32 Dv) {
    switch (D) {
        case 32: return pick_dv<DT, 32>(Dv);
        case 64: return pick_dv<DT, 64>(Dv);
        case 128: return pick_dv<DT, 128>(Dv);
        default: return nullptr;
    }
}

constexpr float LOG2E_F = 1.44269504088896340736f;

// what the two entry points share once their operands are checked: the scale, the dims (256 is a
// dim of the unbiased form; a biased form of it is not built) and the launch
int bias_launch(const char* who, const char* prep, const bsmr_plan* plan, u32 batches, u32 heads,
                const bsmr_attention_operand& Q, const bsmr_attention_operand& K, const bsmr_attention_operand& V,
                const PanelBiasIn& bias, u32 D, u32 Dv, int dtype, const bsmr_attention_operand& O, float* dLse, void* stream) {
    return attn_panels_launch(who, prep, plan, panels_bias_kernel(D, Dv, dtype), batches, heads, Q, K, V, 2u, D, Dv, dtype, 1.0f,
                              LOG2E_F, 1.0f, O, dLse, stream, &bias);
}

int bias_validate(const char* who, u32 D, u32 Dv, int dtype, float scale) {
    float c;
    BSMR_CHECK(attn_validate_scale(who, scale, &c));
    BSMR_CHECK(panel_validate_dims(who, D, Dv, dtype, true));
    if (!panels_bias_kernel(D, Dv, dtype)) {
        set_error(std::string(who) + ": the biased form of D = " + std::to_string(D) + ", Dv = " + std::to_string(Dv) +
                  " is not built (D and Dv each one of 32, 64, 128)");
        return BSMR_ERR_UNSUPPORTED;
    }
    return BSMR_OK;
}

}  // namespace

PanelFn panels_bias_kernel(u32 D, u32 Dv, int dtype) {
    return dtype == BSMR_F16 ? pick_d<BSMR_F16>(D, Dv) : dtype == BSMR_BF16 ? pick_d<BSMR_BF16>(D, Dv) : nullptr;
}

int attn_panels_check_bias(const char* who, const bsmr_plan* plan, const float* dBias, u64 stride) {
    if (!dBias || (reinterpret_cast<uintptr_t>(dBias) & 3u)) {
        set_error(std::string(who) + ": dBias must be non-null and 4-byte aligned");
        return BSMR_ERR_INVALID;
    }
    if (stride != 0 && stride < plan->p.nnz) {
        set_error(std::string(who) + ": bias_slice_stride must be 0 (one bias for all slices) or at least nnz");
        return BSMR_ERR_INVALID;
    }
    return BSMR_OK;
}

}  // namespace bsmr

using namespace bsmr;

extern "C" int bsmr_attention_panels_bias(const bsmr_plan* plan, const void* dQ, const void* dK, const void* dV,
                                          const float* dBias, uint32_t D, uint32_t Dv, int dtype, float scale, float* dO,
                                          float* dLse, void* stream) {
    const char* who = "bsmr_attention_panels_bias";
    BSMR_CHECK(attn_panels_check_dense(who, "dQ, dK, dV and dO", plan, dQ, dK, dV, dO, dLse));
    BSMR_CHECK(attn_panels_check_bias(who, plan, dBias, 0));
    BSMR_CHECK(bias_validate(who, D, Dv, dtype, scale));
    const Plan& p = plan->p;
    return bias_launch(who, "bsmr_plan_prepare_attention_panels_bias", plan, 1, 1, attention_dense_operand(dQ, 1, p.M, D),
                       attention_dense_operand(dK, 1, p.N, D), attention_dense_operand(dV, 1, p.N, Dv),
                       PanelBiasIn{dBias, 0, scale}, D, Dv, dtype, attention_dense_operand(dO, 1, p.M, Dv), dLse, stream);
}

extern "C" int bsmr_attention_panels_bias_heads(const bsmr_plan* plan, uint32_t batches, uint32_t heads,
                                                const bsmr_attention_operand* Q, const bsmr_attention_operand* K,
                                                const bsmr_attention_operand* V, const float* dBias,
                                                uint64_t bias_slice_stride, uint32_t D, uint32_t Dv, int dtype, float scale,
                                                const bsmr_attention_operand* O, float* dLse, void* stream) {
    const char* who = "bsmr_attention_panels_bias_heads";
    BSMR_CHECK(attn_panels_check_heads(who, plan, dLse));
    BSMR_CHECK(attn_panels_check_bias(who, plan, dBias, bias_slice_stride));
    BSMR_CHECK(bias_validate(who, D, Dv, dtype, scale));
    const Plan& p = plan->p;
    BSMR_CHECK(attn_check_operand(who, "Q", Q, batches, heads, p.M, D, 2u, false));
    BSMR_CHECK(attn_check_operand(who, "K", K, batches, heads, p.N, D, 2u, false));
    BSMR_CHECK(attn_check_operand(who, "V", V, batches, heads, p.N, Dv, 2u, false));
    BSMR_CHECK(attn_check_operand(who, "O", O, batches, heads, p.M, Dv, 4u, true));
    return bias_launch(who, "bsmr_plan_prepare_attention_panels_bias_heads", plan, batches, heads, *Q, *K, *V,
                       PanelBiasIn{dBias, bias_slice_stride, scale}, D, Dv, dtype, *O, dLse, stream);
}
