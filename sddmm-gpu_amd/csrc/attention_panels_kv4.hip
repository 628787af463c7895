// attention_panels_kv4.hip — the panel forward of attention_panels.hip over an MXFP4 K / V cache
// (bsmr_attention_panels_kv4; Q fp16 / bf16, K and V e2m1 nibbles with one e8m0 scale per block of
// 32 elements, and one float scale per tensor on top):
//
//   O = v_scale softmax_row(scale k_scale S .* (Q K4^T)) V4,  LSE of that softmax
//
// Format (include/bsmr.h). A row of width W is one record of
// R(W) = round_up(W / 2 + W / 32, 16) bytes (80 at 128, 144 at 256): bytes [0, W / 2) the nibbles,
// element 2 c in the low nibble of byte c; bytes [W / 2, W / 2 + W / 32) the scale byte of each
// 32-element block; zeros up to R. The value of an element is fl_dtype(e2m1 2^(s - 127)), what
// v_cvt_scalef32_pk_{f16,bf16}_fp4 gives for the scale operand with bits s << 23 (panel_mfma.hpp
// mx_scale, widen2_fp4): exact where that product is a normal number of the type, NaN for the whole
// block at s = 0xFF, and s = 0 is 2^-127 like any other exponent (no special meaning: fp16 gives
// signed zeros there, bf16 its subnormals).
//
// Lists, items, the four waves of a workgroup, both transposed products on
// v_mfma_f32_16x16x32_{f16,bf16}, the mask select, the online softmax, the partials and
// k_attention_panels_reduce are the 16-bit form's; v_scale is the e4m3 form's. The nibbles stay
// nibbles until the instruction before the MFMA that consumes them. With r = l & 15 and g = l >> 4:
//   K        lane (i, g) loads the 16 bytes [64 s + 16 g, +16) of the record of tile column i: the
//            32 elements of block 4 s + g, and that block's scale byte (one byte load). Word h of
//            the 16 bytes is widened by four converts into the A operand of one MFMA, so k-step
//            4 s + h of a score covers the elements 128 s + 32 g' + 8 h + e (g' < 4, e < 8): a
//            permutation of the dot product's terms, which the B operand follows. One 16-byte load
//            feeds four k-steps;
//   Q        lane (r, g) keeps Q[row r][128 s + 32 g + 8 h, +8) as the B operand of k-step 4 s + h:
//            the same D / 32 16-byte loads per item, four neighbouring ones per s;
//   in flight  the next step's K records are requested after this step's score MFMAs: D / 32 data
//            registers and D / 128 scale bytes per tile, where the e4m3 form holds D / 8;
//   V stage  the step's 32 V records are staged in LDS as they are, by 16-byte loads and stores
//            (chunk x = 64 u + lane is 16 bytes of record x / (R / 16); R / 16 is 5 or 9, so a lane
//            takes 3 or 5 chunks per step and only the lower 32 lanes the last), records R bytes
//            apart with no padding: 32 R bytes per wave;
//   V read   lane (i, g) reads the 32-bit word 16 n + i of its eight records (the k-slot order of
//            panel_mfma.hpp), eight consecutive output columns 128 n + 8 i + b of each row, and the
//            records' scale byte of block 4 n + i / 4. One convert widens byte c of a row's word
//            into (column 2 c, column 2 c + 1) of that row; per row pair (j, j + 1) and byte two
//            converts and two v_perm_b32 give one register each of the A operands of MFMAs 2 c and
//            2 c + 1: eight ds_read_b32, eight ds_read_u8, 32 converts and 32 permutes feed eight
//            MFMAs. Banks: one instruction reads word (4 g + j)(R / 4) + 16 n + i per lane; R / 4
//            is 20 or 36, both 4 (mod 16), so 4 g (R / 4) is 16 g (mod 64) and the index is
//            16 g + i + const (mod 64): 64 lanes, 64 banks. The scale bytes of one instruction lie
//            in four words per g, 16 g apart (mod 64) again;
//   O        MFMA b of group n leaves lane (r, g) with O[row r][128 n + 32 g + 8 j + b], j = 0 .. 3:
//            per j the eight consecutive columns b = 0 .. 7, two 16-byte stores;
//   v_scale, partials, LSE  the e4m3 form's.
// D and Dv are each 128 or 256. At 64 a record would be 48 bytes against the e4m3 form's 64, and a
// V row has only 8 words, too few for the read mapping (16 lanes i, one word each); 32 likewise.
// Conventions: attention_panels.hip's. A 0xFF scale byte of a K record reaches the rows that store
// the column (the select), one of a V record the rows of the panels whose union holds it.
//
// Resources: 4 x 32 R(Dv) bytes of LDS per workgroup, 10,240 at Dv = 128 and 18,432 at Dv = 256;
// the registers set the occupancy (DESIGN.md section 25's table).
#include <hip/hip_runtime.h>

#include <string>

#include "attention_common.hpp"
#include "attention_layout.hpp"
#include "attention_panels_args.hpp"
#include "panel_mfma.hpp"
#include "plan.hpp"
#include "seg_walk.hpp"  // exp2_hw

namespace bsmr {
namespace {

// bytes of the record of a row of `width` elements
constexpr u32 mx4_record_bytes(u32 width) { return (width / 2u + width / 32u + 15u) & ~15u; }

// waves per SIMD that the register allocator is held to, as in the e4m3 form
constexpr int KV4_WAVES = 2;

// Byte C of the words w of a lane's eight staged rows (k-slot order), widened with the rows' block
// scales: column 2 C of the eight rows (even) and column 2 C + 1 (odd) as A operands of two MFMAs of
// the second product against the lane's packed weights pb
template <int DT, int C>
__device__ __forceinline__ void staged_byte(const u32 (&w)[8], const float (&sc)[8], const uint4& pb, f32x4* acc) {
    u32 x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = widen2_fp4<DT, C>(w[j], sc[j]);
    uint4 even, odd;
    even.x = __builtin_amdgcn_perm(x[1], x[0], 0x05040100u), odd.x = __builtin_amdgcn_perm(x[1], x[0], 0x07060302u);
    even.y = __builtin_amdgcn_perm(x[3], x[2], 0x05040100u), odd.y = __builtin_amdgcn_perm(x[3], x[2], 0x07060302u);
    even.z = __builtin_amdgcn_perm(x[5], x[4], 0x05040100u), odd.z = __builtin_amdgcn_perm(x[5], x[4], 0x07060302u);
    even.w = __builtin_amdgcn_perm(x[7], x[6], 0x05040100u), odd.w = __builtin_amdgcn_perm(x[7], x[6], 0x07060302u);
    acc[2 * C] = mfma32<DT>(even, pb, acc[2 * C]);
    acc[2 * C + 1] = mfma32<DT>(odd, pb, acc[2 * C + 1]);
}

// Group n of the second product from a step's 32 staged records (R bytes apart, W elements each):
// acc[b] gains column 128 n + 8 i + b of the lane's eight rows times pb, b = 0 .. 7
template <int DT, u32 R, u32 W>
__device__ __forceinline__ void staged_oct(const char* tile, u32 n, u32 i, u32 g, const uint4& pb, f32x4* acc) {
    u32 w[8];
    float sc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const char* rec = tile + panel_slot(g, j) * R;
        w[j] = *reinterpret_cast<const u32*>(rec + (16u * n + i) * 4u);
        sc[j] = mx_scale(*reinterpret_cast<const unsigned char*>(rec + W / 2u + 4u * n + (i >> 2)));
    }
    staged_byte<DT, 0>(w, sc, pb, acc);
    staged_byte<DT, 1>(w, sc, pb, acc);
    staged_byte<DT, 2>(w, sc, pb, acc);
    staged_byte<DT, 3>(w, sc, pb, acc);
}

template <int DT, int D, int DV>
__global__ __launch_bounds__(PANEL_WAVES * 64) __attribute__((amdgpu_waves_per_eu(KV4_WAVES)))
void k_attention_panels_kv4(const PanelArgs a) {
    constexpr int KS = D / 128;                         // 16-byte chunks of a K record per lane: four k-steps each
    constexpr int NG = DV / 128;                        // groups of eight output tiles
    constexpr u32 VR = mx4_record_bytes(DV);            // bytes of a V record, and between staged records
    constexpr u32 CPR = VR / 16u;                       // 16-byte chunks per V record
    constexpr u32 CHUNKS = PANEL_STEP_COLS * CPR;       // per step
    constexpr int VLOADS = (CHUNKS + 63u) / 64u;        // per lane and step, the last for the lanes below CHUNKS % 64
    __shared__ __attribute__((aligned(16))) char vstage[PANEL_WAVES][PANEL_STEP_COLS * VR];

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
    uint4 q[4 * KS];
#pragma unroll
    for (int s = 0; s < 4 * KS; ++s)
        q[s] = live ? load16(Qs + static_cast<size_t>(row) * a.Q.row + (128u * (s / 4) + 32u * g + 8u * (s % 4)) * 2u)
                    : make_uint4(0, 0, 0, 0);

    float m = -INFINITY, l = 0.f;
    f32x4 acc[8 * NG];
#pragma unroll
    for (int n = 0; n < 8 * NG; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

    const PanelStep* st = a.steps + it.step0;
    uint4 k0[KS], k1[KS];  // nibbles: block 4 s + g of the two tiles' records
    u32 e0[KS], e1[KS];    // and the blocks' scale bytes
    auto load_k = [&](const PanelStep* sp) {
        const char* r0 = Ks + static_cast<size_t>(sp->cols[r]) * a.K.row;
        const char* r1 = Ks + static_cast<size_t>(sp->cols[16u + r]) * a.K.row;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            k0[s] = load16(r0 + 64u * s + 16u * g);
            k1[s] = load16(r1 + 64u * s + 16u * g);
            e0[s] = *reinterpret_cast<const unsigned char*>(r0 + D / 2 + 4u * s + g);
            e1[s] = *reinterpret_cast<const unsigned char*>(r1 + D / 2 + 4u * s + g);
        }
    };
    if (it.nsteps) load_k(st);
    for (u32 step = 0; step < it.nsteps; ++step, ++st) {
        const u32 colv = st->cols[lane & 31u];  // lane x holds step column x & 31
        const u32 mask = st->masks[r];
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const float f0 = mx_scale(e0[s]), f1 = mx_scale(e1[s]);
            s0 = mfma32<DT>(widen8_fp4<DT>(k0[s].x, f0), q[4 * s], s0);
            s1 = mfma32<DT>(widen8_fp4<DT>(k1[s].x, f1), q[4 * s], s1);
            s0 = mfma32<DT>(widen8_fp4<DT>(k0[s].y, f0), q[4 * s + 1], s0);
            s1 = mfma32<DT>(widen8_fp4<DT>(k1[s].y, f1), q[4 * s + 1], s1);
            s0 = mfma32<DT>(widen8_fp4<DT>(k0[s].z, f0), q[4 * s + 2], s0);
            s1 = mfma32<DT>(widen8_fp4<DT>(k1[s].z, f1), q[4 * s + 2], s1);
            s0 = mfma32<DT>(widen8_fp4<DT>(k0[s].w, f0), q[4 * s + 3], s0);
            s1 = mfma32<DT>(widen8_fp4<DT>(k1[s].w, f1), q[4 * s + 3], s1);
        }
        if (step + 1 < it.nsteps) load_k(st + 1);

        // the step's V records into LDS as they are: chunk x = 64 u + lane is 16 bytes of record
        // x / CPR; chunks at and past CHUNKS do not exist. The reads of the step before are done first
        wave_lds_sync();
        {
            uint4 v[VLOADS];
#pragma unroll
            for (int u = 0; u < VLOADS; ++u) {
                const u32 x = 64u * u + lane;
                const u32 col = __shfl(colv, static_cast<int>((x / CPR) & 31u));
                if (x < CHUNKS) v[u] = load16(Vs + static_cast<size_t>(col) * a.V.row + (x % CPR) * 16u);
            }
#pragma unroll
            for (int u = 0; u < VLOADS; ++u) {
                const u32 x = 64u * u + lane;
                if (x < CHUNKS) *reinterpret_cast<uint4*>(vl + x * 16u) = v[u];
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
        for (int n = 0; n < 8 * NG; ++n) acc[n] *= f;

        wave_lds_sync();
#pragma unroll
        for (int n = 0; n < NG; ++n) staged_oct<DT, VR, DV>(vl, n, r, g, pb, acc + 8 * n);
    }

    // the row's four lanes in g order: every lane of the row ends with the same sum
    const float lt = ((__shfl(l, static_cast<int>(r)) + __shfl(l, static_cast<int>(16u + r))) +
                      __shfl(l, static_cast<int>(32u + r))) + __shfl(l, static_cast<int>(48u + r));
    if (!live) return;
    // acc[8 n + b][j] is column 128 n + 32 g + 8 j + b of the row
    if (it.part == PANEL_DIRECT) {
        const float inv = inverse_of(lt) * a.vscale;
        float* o = reinterpret_cast<float*>(Os + static_cast<size_t>(row) * a.O.row) + 32u * g;
#pragma unroll
        for (int n = 0; n < NG; ++n)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4* c = acc + 8 * n;
                *reinterpret_cast<float4*>(o + 128 * n + 8 * j) = make_float4(c[0][j] * inv, c[1][j] * inv, c[2][j] * inv, c[3][j] * inv);
                *reinterpret_cast<float4*>(o + 128 * n + 8 * j + 4) =
                    make_float4(c[4][j] * inv, c[5][j] * inv, c[6][j] * inv, c[7][j] * inv);
            }
        if (g == 0 && a.lse) a.lse[slice * a.M + row] = m * a.scale + logf(lt);
    } else {
        const size_t slot = (slice * a.partials + it.part) * PANEL_ROWS + r;
        float* o = a.pacc + slot * DV + 32u * g;
#pragma unroll
        for (int n = 0; n < NG; ++n)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4* c = acc + 8 * n;
                *reinterpret_cast<float4*>(o + 128 * n + 8 * j) = make_float4(c[0][j], c[1][j], c[2][j], c[3][j]);
                *reinterpret_cast<float4*>(o + 128 * n + 8 * j + 4) = make_float4(c[4][j], c[5][j], c[6][j], c[7][j]);
            }
        if (g == 0) {
            a.pml[2u * slot] = m;
            a.pml[2u * slot + 1u] = lt;
        }
    }
}

template <int DT>
PanelFn pick(u32 D, u32 Dv) {
    if (D == 128) return Dv == 128 ? k_attention_panels_kv4<DT, 128, 128> : Dv == 256 ? k_attention_panels_kv4<DT, 128, 256> : nullptr;
    if (D == 256) return Dv == 128 ? k_attention_panels_kv4<DT, 256, 128> : Dv == 256 ? k_attention_panels_kv4<DT, 256, 256> : nullptr;
    return nullptr;
}

// The argument rules the two entry points share. UNSUPPORTED: a Q dtype other than fp16 / bf16, D or
// Dv outside {128, 256}. The scales: attn_panels_kv_scales
int kv4_validate(const char* who, u32 D, u32 Dv, int dtype, float scale, float k_scale, float v_scale, float* eff, float* c,
                 PanelFn* fn) {
    *fn = dtype == BSMR_F16 ? pick<BSMR_F16>(D, Dv) : dtype == BSMR_BF16 ? pick<BSMR_BF16>(D, Dv) : nullptr;
    if (!*fn) {
        set_error(std::string(who) + ": dtype must be BSMR_F16 or BSMR_BF16 and D and Dv each one of 128, 256");
        return BSMR_ERR_UNSUPPORTED;
    }
    return attn_panels_kv_scales(who, scale, k_scale, v_scale, eff, c);
}

}  // namespace
}  // namespace bsmr

using namespace bsmr;

extern "C" int bsmr_attention_panels_kv4(const bsmr_plan* plan, const void* dQ, const void* dK4, const void* dV4, uint32_t D,
                                         uint32_t Dv, int dtype, float scale, float k_scale, float v_scale, float* dO,
                                         float* dLse, void* stream) {
    const char* who = "bsmr_attention_panels_kv4";
    BSMR_CHECK(attn_panels_check_dense(who, "dQ, dK4, dV4 and dO", plan, dQ, dK4, dV4, dO, dLse));
    float eff, c;
    PanelFn fn;
    BSMR_CHECK(kv4_validate(who, D, Dv, dtype, scale, k_scale, v_scale, &eff, &c, &fn));
    const Plan& p = plan->p;
    return attn_panels_launch(who, "bsmr_plan_prepare_attention_panels", plan, fn, 1, 1, attention_dense_operand(dQ, 1, p.M, D),
                              attention_dense_operand(dK4, 1, p.N, mx4_record_bytes(D)),
                              attention_dense_operand(dV4, 1, p.N, mx4_record_bytes(Dv)), 1u, D, Dv, dtype, eff, c, v_scale,
                              attention_dense_operand(dO, 1, p.M, Dv), dLse, stream);
}

extern "C" int bsmr_attention_panels_kv4_heads(const bsmr_plan* plan, uint32_t batches, uint32_t heads,
                                               const bsmr_attention_operand* Q, const bsmr_attention_operand* K4,
                                               const bsmr_attention_operand* V4, uint32_t D, uint32_t Dv, int dtype,
                                               float scale, float k_scale, float v_scale, const bsmr_attention_operand* O,
                                               float* dLse, void* stream) {
    const char* who = "bsmr_attention_panels_kv4_heads";
    BSMR_CHECK(attn_panels_check_heads(who, plan, dLse));
    float eff, c;
    PanelFn fn;
    BSMR_CHECK(kv4_validate(who, D, Dv, dtype, scale, k_scale, v_scale, &eff, &c, &fn));
    const Plan& p = plan->p;
    BSMR_CHECK(attn_check_operand(who, "Q", Q, batches, heads, p.M, D, 2u, false));
    BSMR_CHECK(attn_check_operand(who, "K4", K4, batches, heads, p.N, mx4_record_bytes(D), 1u, false));
    BSMR_CHECK(attn_check_operand(who, "V4", V4, batches, heads, p.N, mx4_record_bytes(Dv), 1u, false));
    BSMR_CHECK(attn_check_operand(who, "O", O, batches, heads, p.M, Dv, 4u, true));
    return attn_panels_launch(who, "bsmr_plan_prepare_attention_panels_heads", plan, fn, batches, heads, *Q, *K4, *V4, 1u, D, Dv,
                              dtype, eff, c, v_scale, *O, dLse, stream);
}
