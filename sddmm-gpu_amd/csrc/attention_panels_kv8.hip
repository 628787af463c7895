// attention_panels_kv8.hip — the panel forward of attention_panels.hip over an fp8 K / V cache
// (bsmr_attention_panels_kv8; Q fp16 / bf16, K and V OCP e4m3 bytes with one scale each):
//
//   O = v_scale softmax_row(scale k_scale S .* (Q K8^T)) V8,  LSE of that softmax
//
// Lists, items, the four waves of a workgroup, both transposed products on
// v_mfma_f32_16x16x32_{f16,bf16}, the mask select, the online softmax, the partials and
// k_attention_panels_reduce are the 16-bit form's. K and V stay bytes until the instruction before
// the MFMA that consumes them: the packed convert (panel_mfma.hpp widen2) is exact, so the MFMAs
// see the operands the 16-bit form would see on widened tensors, and what changes is how the bytes
// travel. With r = l & 15 and g = l >> 4:
//   K        lane (i, g) loads the 16 bytes [64 s + 16 g, +16) of the K row of tile column i: one
//            16-byte load per tile and *two* k-steps, half the bytes per k-step of the 16-bit form.
//            The two words [64 s + 16 g, +8) are widened into the A operand of one MFMA and the two
//            words [64 s + 16 g + 8, +8) into that of the next, so k-step 2 s + h of a score covers
//            the elements 64 s + 16 g' + 8 h + e (g' < 4, e < 8): a permutation of the dot
//            product's terms, which the B operand follows;
//   Q        lane (r, g) keeps Q[row r][64 s + 16 g + 8 h, +8) as the B operand of k-step 2 s + h:
//            the same D / 32 16-byte loads per item, two neighbouring ones per s;
//   in flight  the next step's K rows are requested after this step's score MFMAs, as bytes: D / 8
//            registers where the 16-bit form holds D / 4;
//   V stage  the step's 32 V rows are staged as bytes by 16-byte loads and stores (chunk
//            x = 64 u + lane is 16 bytes of row x / (Dv / 16): each row is fetched once per step),
//            rows Dv + 16 bytes apart: 32 (Dv + 16) bytes per wave, against 32 (2 Dv + 16);
//   V read   lane (i, g) reads the 32-bit word 16 n + i of its eight rows (the k-slot order of
//            panel_mfma.hpp): four consecutive output columns
//            64 n + 4 i + b of each row. Per row pair two v_perm_b32 re-deal the two words into
//            (row j, row j + 1) byte pairs, b = 0, 1 in one word and b = 2, 3 in the other, and the
//            packed convert widens each pair into one register of the A operand of MFMA b: eight
//            ds_read_b32, eight permutes and sixteen converts feed four MFMAs (the 16-bit form:
//            eight reads and eight permutes for two). Banks: one instruction reads word
//            (4 g + j)(Dv / 4 + 4) + 16 n + i per lane; Dv / 4 is a multiple of 16, so 4 g (Dv / 4)
//            is a multiple of 64 and the index is 16 g + i + const (mod 64): 64 lanes, 64 banks.
//            (A padding of 4 or 12 words mod 16 does that; 16 bytes also keeps the rows aligned for
//            the 16-byte stores.) Dv = 32 has only 8 words per row and is not built;
//   O        MFMA b of group n leaves lane (r, g) with O[row r][64 n + 16 g + 4 j + b], j = 0 .. 3:
//            over b and j the 16 consecutive columns [64 n + 16 g, +16), four 16-byte stores;
//   v_scale  once per row: inv = (1 / l) v_scale, a rounded product, then acc inv; the reduce does
//            the same for a split panel (PanelArgs::vscale).
// Conventions: attention_panels.hip's. e4m3 has NaN and no inf: a NaN byte of a K row reaches the
// rows that store the column (the select), one of a V row the rows of the panels whose union holds it.
//
// Resources: 4 x 32 (Dv + 16) bytes of LDS per workgroup: 34 KiB at Dv = 256, four workgroups per
// CU where the 16-bit form fits two; there the registers, not LDS, set the occupancy (KV8_WAVES).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "attention_common.hpp"
#include "attention_layout.hpp"
#include "attention_panels_args.hpp"
#include "panel_mfma.hpp"
#include "plan.hpp"
#include "seg_walk.hpp"  // exp2_hw

namespace bsmr {
namespace {

// bytes between the staged rows of `width` e4m3 elements (the header comment's bank arithmetic)
constexpr u32 staged_row_bytes8(u32 width) { return width + 16u; }

// Waves per SIMD that the register allocator is held to: 2, as in the 16-bit form. The halved V
// stage would let four workgroups of Dv = 256 share a CU (4 waves per SIMD, 128 registers), but the
// registers do not follow: held to 4 waves the (64, 256) form spills 25 registers and held to 3 the
// (128, 256) form spills 3 (acc alone is Dv / 4 = 64, V in flight 32, the four operands 16). Left
// at 2, the forms take what they need and run at 2 to 5 waves per SIMD (DESIGN.md §20's table)
constexpr int KV8_WAVES = 2;

// The A operands of four MFMAs of the second product from a step's 32 staged e4m3 rows (ROW bytes
// apart): op[b] is element 64 n + 4 i + b of the lane's eight rows, widened
template <int DT, u32 ROW>
__device__ __forceinline__ void staged_quad(const char* tile, u32 n, u32 i, u32 g, uint4 (&op)[4]) {
    u32 w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = *reinterpret_cast<const u32*>(tile + panel_slot(g, j) * ROW + (16u * n + i) * 4u);
    u32 lo[4], hi[4];  // per row pair: bytes (b0, b0', b1, b1') and (b2, b2', b3, b3')
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        lo[jj] = __builtin_amdgcn_perm(w[2 * jj + 1], w[2 * jj], 0x05010400u);
        hi[jj] = __builtin_amdgcn_perm(w[2 * jj + 1], w[2 * jj], 0x07030602u);
    }
    op[0] = make_uint4(widen2<DT, false>(lo[0]), widen2<DT, false>(lo[1]), widen2<DT, false>(lo[2]), widen2<DT, false>(lo[3]));
    op[1] = make_uint4(widen2<DT, true>(lo[0]), widen2<DT, true>(lo[1]), widen2<DT, true>(lo[2]), widen2<DT, true>(lo[3]));
    op[2] = make_uint4(widen2<DT, false>(hi[0]), widen2<DT, false>(hi[1]), widen2<DT, false>(hi[2]), widen2<DT, false>(hi[3]));
    op[3] = make_uint4(widen2<DT, true>(hi[0]), widen2<DT, true>(hi[1]), widen2<DT, true>(hi[2]), widen2<DT, true>(hi[3]));
}

template <int DT, int D, int DV>
__global__ __launch_bounds__(PANEL_WAVES * 64) __attribute__((amdgpu_waves_per_eu(KV8_WAVES)))
void k_attention_panels_kv8(const PanelArgs a) {
    constexpr int KS = D / 64;                   // pairs of k-steps of a score tile
    constexpr int NQ = DV / 64;                  // groups of four output tiles
    constexpr u32 VROW = staged_row_bytes8(DV);  // bytes between staged V rows
    constexpr u32 CPR = DV / 16;                 // 16-byte chunks per V row
    constexpr int VLOADS = DV / 32;              // chunks per lane and step (32 rows)
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
    char* vl = vstage[wave];

    const u32 r = lane & 15u, g = lane >> 4;
    const bool live = it.row0 + r < a.M;  // (a row of a short last panel is neither loaded nor stored)
    const u32 row = live ? a.rows[it.row0 + r] : 0u;
    uint4 q[2 * KS];
#pragma unroll
    for (int s = 0; s < 2 * KS; ++s)
        q[s] = live ? load16(Qs + static_cast<size_t>(row) * a.Q.row + (64u * (s / 2) + 16u * g + 8u * (s % 2)) * 2u)
                    : make_uint4(0, 0, 0, 0);

    float m = -INFINITY, l = 0.f;
    f32x4 acc[4 * NQ];
#pragma unroll
    for (int n = 0; n < 4 * NQ; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

    const PanelStep* st = a.steps + it.step0;
    uint4 k0[KS], k1[KS];  // e4m3 bytes
    auto load_k = [&](const PanelStep* sp) {
        const u32 c0 = sp->cols[r], c1 = sp->cols[16u + r];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            k0[s] = load16(Ks + static_cast<size_t>(c0) * a.K.row + 64u * s + 16u * g);
            k1[s] = load16(Ks + static_cast<size_t>(c1) * a.K.row + 64u * s + 16u * g);
        }
    };
    if (it.nsteps) load_k(st);
    for (u32 step = 0; step < it.nsteps; ++step, ++st) {
        const u32 colv = st->cols[lane & 31u];  // lane x holds step column x & 31
        const u32 mask = st->masks[r];
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            s0 = mfma32<DT>(widen8<DT>(k0[s].x, k0[s].y), q[2 * s], s0);
            s1 = mfma32<DT>(widen8<DT>(k1[s].x, k1[s].y), q[2 * s], s1);
            s0 = mfma32<DT>(widen8<DT>(k0[s].z, k0[s].w), q[2 * s + 1], s0);
            s1 = mfma32<DT>(widen8<DT>(k1[s].z, k1[s].w), q[2 * s + 1], s1);
        }
        if (step + 1 < it.nsteps) load_k(st + 1);

        // the step's V rows into LDS as bytes: chunk x = 64 u + lane is 16 bytes of row x / CPR. The
        // reads of the step before are done first
        wave_lds_sync();
        {
            uint4 v[VLOADS];
#pragma unroll
            for (int u = 0; u < VLOADS; ++u) {
                const u32 x = 64u * u + lane;
                const u32 col = __shfl(colv, static_cast<int>(x / CPR));
                v[u] = load16(Vs + static_cast<size_t>(col) * a.V.row + (x % CPR) * 16u);
            }
#pragma unroll
            for (int u = 0; u < VLOADS; ++u) {
                const u32 x = 64u * u + lane;
                *reinterpret_cast<uint4*>(vl + (x / CPR) * VROW + (x % CPR) * 16u) = v[u];
            }
        }

        // masked scores of the lane's row, the step's maximum and the weights
        float p[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            p[j] = (mask >> panel_slot(g, j)) & 1u ? s0[j] : -INFINITY;
            p[4 + j] = (mask >> panel_slot(g, 4 + j)) & 1u ? s1[j] : -INFINITY;
        }
        float ms = p[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) ms = fmaxf(ms, p[j]);
        ms = fmaxf(ms, __shfl_xor(ms, 16));
        ms = fmaxf(ms, __shfl_xor(ms, 32));
        const float mn = fmaxf(m, ms);
        const float shift = shift_of(mn);
        const float f = exp2_hw((m - shift) * a.c);
        m = mn;
        float t[8], ts = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            t[j] = exp2_hw((p[j] - shift) * a.c);
            ts += t[j];
        }
        l = l * f + ts;
        const uint4 pb = pack8<DT>(t);
#pragma unroll
        for (int n = 0; n < 4 * NQ; ++n) acc[n] *= f;

        wave_lds_sync();
#pragma unroll
        for (int n = 0; n < NQ; ++n) {
            uint4 op[4];
            staged_quad<DT, VROW>(vl, n, r, g, op);
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[4 * n + b] = mfma32<DT>(op[b], pb, acc[4 * n + b]);
        }
    }

    // the row's four lanes in g order: every lane of the row ends with the same sum
    const float lt = ((__shfl(l, static_cast<int>(r)) + __shfl(l, static_cast<int>(16u + r))) +
                      __shfl(l, static_cast<int>(32u + r))) + __shfl(l, static_cast<int>(48u + r));
    if (!live) return;
    // acc[4 n + b][j] is column 64 n + 16 g + 4 j + b of the row
    if (it.part == PANEL_DIRECT) {
        const float inv = inverse_of(lt) * a.vscale;
        float* o = reinterpret_cast<float*>(Os + static_cast<size_t>(row) * a.O.row) + 16u * g;
#pragma unroll
        for (int n = 0; n < NQ; ++n)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                *reinterpret_cast<float4*>(o + 64 * n + 4 * j) = make_float4(acc[4 * n][j] * inv, acc[4 * n + 1][j] * inv,
                                                                             acc[4 * n + 2][j] * inv, acc[4 * n + 3][j] * inv);
        if (g == 0 && a.lse) a.lse[slice * a.M + row] = m * a.scale + logf(lt);
    } else {
        const size_t slot = (slice * a.partials + it.part) * PANEL_ROWS + r;
        float* o = a.pacc + slot * DV + 16u * g;
#pragma unroll
        for (int n = 0; n < NQ; ++n)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                *reinterpret_cast<float4*>(o + 64 * n + 4 * j) =
                    make_float4(acc[4 * n][j], acc[4 * n + 1][j], acc[4 * n + 2][j], acc[4 * n + 3][j]);
        if (g == 0) {
            a.pml[2u * slot] = m;
            a.pml[2u * slot + 1u] = lt;
        }
    }
}

template <int DT, int D>
PanelFn pick_dv(u32 Dv) {
    switch (Dv) {
        case 64: return k_attention_panels_kv8<DT, D, 64>;
        case 128: return k_attention_panels_kv8<DT, D, 128>;
        case 256: return k_attention_panels_kv8<DT, D, 256>;
        default: return nullptr;
    }
}

template <int DT>
PanelFn pick_d(u32 D, u32 Dv) {
    switch (D) {
        case 64: return pick_dv<DT, 64>(Dv);
        case 128: return pick_dv<DT, 128>(Dv);
        case 256: return pick_dv<DT, 256>(Dv);
        default: return nullptr;
    }
}

// The argument rules the two entry points share. UNSUPPORTED: a Q dtype other than fp16 / bf16, D or
// Dv outside the built forms, another K / V format. The scales, *eff and *c: attn_panels_kv_scales
int kv8_validate(const char* who, u32 D, u32 Dv, int dtype, int kv_dtype, float scale, float k_scale, float v_scale,
                 float* eff, float* c, PanelFn* fn) {
    *fn = dtype == BSMR_F16 ? pick_d<BSMR_F16>(D, Dv) : dtype == BSMR_BF16 ? pick_d<BSMR_BF16>(D, Dv) : nullptr;
    if (!*fn || kv_dtype != BSMR_KV_F8_E4M3) {
        set_error(std::string(who) + ": dtype must be BSMR_F16 or BSMR_BF16, D and Dv each one of 64, 128, 256 and kv_dtype "
                                     "BSMR_KV_F8_E4M3");
        return BSMR_ERR_UNSUPPORTED;
    }
    return attn_panels_kv_scales(who, scale, k_scale, v_scale, eff, c);
}

}  // namespace
}  // namespace bsmr

using namespace bsmr;

extern "C" int bsmr_attention_panels_kv8(const bsmr_plan* plan, const void* dQ, const void* dK8, const void* dV8, uint32_t D,
                                         uint32_t Dv, int dtype, int kv_dtype, float scale, float k_scale, float v_scale,
                                         float* dO, float* dLse, void* stream) {
    const char* who = "bsmr_attention_panels_kv8";
    BSMR_CHECK(attn_panels_check_dense(who, "dQ, dK8, dV8 and dO", plan, dQ, dK8, dV8, dO, dLse));
    float eff, c;
    PanelFn fn;
    BSMR_CHECK(kv8_validate(who, D, Dv, dtype, kv_dtype, scale, k_scale, v_scale, &eff, &c, &fn));
    const Plan& p = plan->p;
    return attn_panels_launch(who, "bsmr_plan_prepare_attention_panels", plan, fn, 1, 1, attention_dense_operand(dQ, 1, p.M, D),
                              attention_dense_operand(dK8, 1, p.N, D), attention_dense_operand(dV8, 1, p.N, Dv), 1u, D, Dv,
                              dtype, eff, c, v_scale, attention_dense_operand(dO, 1, p.M, Dv), dLse, stream);
}

extern "C" int bsmr_attention_panels_kv8_heads(const bsmr_plan* plan, uint32_t batches, uint32_t heads,
                                               const bsmr_attention_operand* Q, const bsmr_attention_operand* K8,
                                               const bsmr_attention_operand* V8, uint32_t D, uint32_t Dv, int dtype,
                                               int kv_dtype, float scale, float k_scale, float v_scale,
                                               const bsmr_attention_operand* O, float* dLse, void* stream) {
    const char* who = "bsmr_attention_panels_kv8_heads";
    BSMR_CHECK(attn_panels_check_heads(who, plan, dLse));
    float eff, c;
    PanelFn fn;
    BSMR_CHECK(kv8_validate(who, D, Dv, dtype, kv_dtype, scale, k_scale, v_scale, &eff, &c, &fn));
    const Plan& p = plan->p;
    BSMR_CHECK(attn_check_operand(who, "Q", Q, batches, heads, p.M, D, 2u, false));
    BSMR_CHECK(attn_check_operand(who, "K8", K8, batches, heads, p.N, D, 1u, false));
    BSMR_CHECK(attn_check_operand(who, "V8", V8, batches, heads, p.N, Dv, 1u, false));
    BSMR_CHECK(attn_check_operand(who, "O", O, batches, heads, p.M, Dv, 4u, true));
    return attn_panels_launch(who, "bsmr_plan_prepare_attention_panels_heads", plan, fn, batches, heads, *Q, *K8, *V8, 1u, D, Dv,
                              dtype, eff, c, v_scale, *O, dLse, stream);
}
