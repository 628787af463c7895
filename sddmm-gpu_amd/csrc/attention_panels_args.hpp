// attention_panels_args.hpp — what the forms of the panel attention forward share: the kernels'
// argument record, the softmax conventions and the one launch routine (attention_panels.hip, the
// 16-bit K / V form and the reduce; attention_panels_kv8.hip, the e4m3 K / V form;
// attention_panels_kv4.hip, the MXFP4 K / V form).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "attention_common.hpp"
#include "attention_panels.hpp"

namespace bsmr {

struct PanelArgs {
    const PanelItem* items;
    const PanelStep* steps;
    const u32* rows;
    AttnOpBytes Q, K, V, O;  // strides in bytes
    float* lse;              // slices x M, or null
    float* pacc;             // slices x partials x 16 x Dv
    float* pml;              // behind them: slices x partials x 16 x (m, l)
    u32 partials, heads, M, nItems;
    float c, scale;  // scale log2(e), rounded once from double; scale
    float vscale;    // multiplies 1 / l once, rounded, before the product with acc (1: the 16-bit form)
    // the biased form only (attention_panels_bias.hip; null / 0 elsewhere): the rows side's entry
    // positions (spmm_panels.hpp), the bias with its slice stride in elements (0: one for all slices)
    // and the scale of the scores; c is then log2(e) and scale 1, the softmax running in x's units
    const u32* base;
    const u32* pos;
    const float* bias;
    u64 biasStride;
    float xscale;
};

// the per-entry bias of a biased launch: nnz fp32 values at CSR positions per slice
struct PanelBiasIn {
    const float* bias;
    u64 stride;   // elements between the slices' biases; 0: one bias shared by all slices
    float scale;  // the scale of the scores
};

using PanelFn = void (*)(const PanelArgs);

// attention.hip's conventions
__device__ __forceinline__ float shift_of(float m) { return m == -INFINITY ? 0.f : m; }
__device__ __forceinline__ float inverse_of(float s) { return s == 0.f ? 0.f : 1.0f / s; }

// The first checks of a dense entry point (a null plan, a null pointer, alignment; `names` is the
// message's list of the four pointers) and of a heads entry point (a null plan, dLse's alignment);
// else BSMR_ERR_INVALID with the message set. Defined in attention_panels.hip
int attn_panels_check_dense(const char* who, const char* names, const bsmr_plan* plan, const void* dQ, const void* dK,
                            const void* dV, const void* dO, const float* dLse);
int attn_panels_check_heads(const char* who, const bsmr_plan* plan, const float* dLse);

// The launches of a panel forward, arguments already validated: `fn` over the plan's items, then
// k_attention_panels_reduce over its split panels. K and V hold elements of kvBytes bytes; the
// lists and the scratch are built first unless `stream` is capturing (BSMR_ERR_NOT_PREPARED, naming
// `prep`). With `bias` (the biased form: c is log2(e) and scale 1) the rows side's entry positions
// are built with them. Defined in attention_panels.hip
int attn_panels_launch(const char* who, const char* prep, const bsmr_plan* plan, PanelFn fn, u32 batches, u32 heads,
                       const bsmr_attention_operand& Q, const bsmr_attention_operand& K, const bsmr_attention_operand& V,
                       u32 kvBytes, u32 D, u32 Dv, int dtype, float scale, float c, float vscale,
                       const bsmr_attention_operand& O, float* dLse, void* stream, const PanelBiasIn* bias = nullptr);

// The scale rules of the quantised K / V forms (kv8, kv4). INVALID: a k_scale or v_scale that is not
// finite and > 0, or an effective score scale scale k_scale (the exact double product of the two
// floats) that attn_validate_scale's rule refuses. *eff is that product rounded once to float and *c
// its product with log2(e), rounded once from double
inline int attn_panels_kv_scales(const char* who, float scale, float k_scale, float v_scale, float* eff, float* c) {
    if (!(k_scale > 0.f) || !std::isfinite(k_scale) || !(v_scale > 0.f) || !std::isfinite(v_scale)) {
        set_error(std::string(who) + ": k_scale and v_scale must be finite and > 0");
        return BSMR_ERR_INVALID;
    }
    const double e = static_cast<double>(scale) * static_cast<double>(k_scale);
    *eff = static_cast<float>(e);
    *c = static_cast<float>(e * 1.4426950408889634);
    if (!(scale > 0.f) || !std::isfinite(scale) || !(*eff > 0.f) || !std::isfinite(*eff) || !std::isfinite(*c)) {
        set_error(std::string(who) + ": scale and scale * k_scale must be finite and > 0 (and scale * k_scale * log2(e) finite)");
        return BSMR_ERR_INVALID;
    }
    return BSMR_OK;
}

// the biased form's checks of dBias and its stride, and its kernel for (D, Dv, dtype): null where the
// form is not built. Defined in attention_panels_bias.hip
PanelFn panels_bias_kernel(u32 D, u32 Dv, int dtype);
int attn_panels_check_bias(const char* who, const bsmr_plan* plan, const float* dBias, u64 stride);

}  // namespace bsmr
