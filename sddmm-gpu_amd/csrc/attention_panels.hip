// attention_panels.hip — fused sparse attention forward for gfx950 on matrix instructions, per
// 16-row panel of the plan's reordered rows (bsmr_attention_panels; fp16 / bf16 operands):
//
//   O[i,:] = sum_e W_e V[j_e,:],  W = softmax over row i of scale dot(Q[i,:], K[j_e,:])
//
// The gather kernel (attention.hip) loads a K row and a V row per entry. Here a wave takes an item
// (attention_panels.hpp): up to PANEL_ITEM_STEPS steps of 32 columns of one panel's column union,
// and loads every K and V row of the union once for the panel's 16 rows. Both products run on
// v_mfma_f32_16x16x32_{f16,bf16}, transposed, so that every per-row quantity of query row r lives
// on the lanes l with (l & 15) == r and nothing is shuffled between the two products. The lane
// mapping, the k-slot order and the stage layout with its bank arithmetic are panel_mfma.hpp's.
// With r = l & 15 and g = l >> 4:
//   Q        lane (r, g) keeps Q[row r][32 s + 8 g, +8) of every k-step s in registers (D / 32
//            16-byte loads for the whole item; a row past a short panel's end is zeros);
//   scores   per step and 16-column tile, S^T = K_tile Q^T: the A operand of lane (i, g) is the
//            gathered K row of tile column i, elements [32 s + 8 g, +8) (a 16-byte load from L2;
//            the next step's K rows are requested as soon as this step's score MFMAs are issued),
//            the B operand the Q registers. Lane (r, g) gets the scores of its own row at step
//            columns 4 g + j (tile 0) and 16 + 4 g + j (tile 1), j = 0 .. 3;
//   mask     a select per score on bit (column) of the row's 32-bit mask: -inf where the row does
//            not store the column, whatever the product was (a NaN of another row's K row too);
//   softmax  online, per row: the step's maximum over the lane's eight scores and the two xor
//            steps 16 and 32; m' = max(m, m_step); f = 2^((m - m') c), t = 2^((p - m') c) with
//            c = scale log2(e) rounded once from double; shift_of as in attention.hip, so a row
//            that has seen only -inf keeps m = -inf, l = 0, acc = 0. A lane's l holds the fp32 t
//            of its own eight columns per step (l = l f + sum t, in column order); the four lanes
//            of a row are added in g order at the end;
//   O        O^T += V^T P^T per 16 columns of Dv: the B operand is the lane's eight t rounded to
//            the operand type (pack8), the A operand V[those eight columns][dv] out of the step's
//            32 staged V rows (staged_pair). Lane (r, g) then holds O[row r][32 n + 8 g, +8): the
//            row's rescale by f, the final 1 / l and two 16-byte stores per pair sit on the lane
//            that owns the row.
// An item that is its panel's only one stores acc / l and m scale + ln l; an item of a split
// panel stores (m, l, acc) per row to plan-owned scratch and k_attention_panels_reduce combines
// the items as k_attention_reduce does: M = max m_i, every partial scaled once by 2^((m_i - M) c)
// (a rounded product), added in item order. No atomics; the order is a function of the panel's
// column union alone.
//
// Conventions: bsmr_attention's, but for a NaN or inf in a V row, which reaches every row of the
// panels whose column union holds that column (0 x NaN inside the MFMA is NaN) and no row of any
// other panel.
//
// Resources: four waves per workgroup, one item each, with 32 (2 Dv + 16) bytes of LDS per wave
// (66 KiB per workgroup at Dv = 256: two workgroups per CU, two waves per SIMD, which is what
// amdgpu_waves_per_eu(2) lets the register allocator count on: 256 VGPRs).
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <string>
#include <vector>

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

template <int DT, int D, int DV>
__global__ __launch_bounds__(PANEL_WAVES * 64) __attribute__((amdgpu_waves_per_eu(2)))
void k_attention_panels(const PanelArgs a) {
    constexpr int KS = D / 32;                // k-steps of a score tile
    constexpr int NP = DV / 32;               // pairs of output tiles
    constexpr u32 VROW = staged_row_bytes(DV);  // bytes between staged V rows
    constexpr u32 CPR = DV / 8;               // 16-byte chunks per V row
    constexpr int VLOADS = DV / 16;           // chunks per lane and step (32 rows)
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
    uint4 k0[KS], k1[KS];
    auto load_k = [&](const PanelStep* sp) {
        const u32 c0 = sp->cols[r], c1 = sp->cols[16u + r];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            k0[s] = load16(Ks + static_cast<size_t>(c0) * a.K.row + (32u * s + 8u * g) * 2u);
            k1[s] = load16(Ks + static_cast<size_t>(c1) * a.K.row + (32u * s + 8u * g) * 2u);
        }
    };
    if (it.nsteps) load_k(st);
    for (u32 step = 0; step < it.nsteps; ++step, ++st) {
        const u32 colv = st->cols[lane & 31u];  // lane x holds step column x & 31
        const u32 mask = st->masks[r];
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            s0 = mfma32<DT>(k0[s], q[s], s0);
            s1 = mfma32<DT>(k1[s], q[s], s1);
        }
        if (step + 1 < it.nsteps) load_k(st + 1);

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
        for (int n = 0; n < 2 * NP; ++n) acc[n] *= f;

        wave_lds_sync();
#pragma unroll
        for (int n = 0; n < NP; ++n) {
            uint4 even, odd;
            staged_pair<VROW>(vl, n, r, g, even, odd);
            acc[2 * n] = mfma32<DT>(even, pb, acc[2 * n]);
            acc[2 * n + 1] = mfma32<DT>(odd, pb, acc[2 * n + 1]);
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
        if (g == 0 && a.lse) a.lse[slice * a.M + row] = m * a.scale + logf(lt);
    } else {
        const size_t slot = (slice * a.partials + it.part) * PANEL_ROWS + r;
        store_acc<NP>(a.pacc + slot * DV + 8u * g, acc);
        if (g == 0) {
            a.pml[2u * slot] = m;
            a.pml[2u * slot + 1u] = lt;
        }
    }
}

// a split panel's rows: M = max m_i, then every partial scaled once by f_i = 2^((m_i - M) c) (a
// rounded product each, never fused into the sum) and added in item order; one thread per row and
// four columns
__global__ __launch_bounds__(256) void k_attention_panels_reduce(const PanelArgs a, const PanelRed* reds, u32 nReds, u32 Dv) {
#pragma clang fp contract(off)
    const u32 head = blockIdx.y, bat = blockIdx.z;
    const size_t slice = static_cast<size_t>(bat) * a.heads + head;
    char* O = attn_slice_base(a.O, bat, head);
    const u32 q4 = Dv / 4u;
    const size_t t = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
    if (t >= static_cast<size_t>(nReds) * PANEL_ROWS * q4) return;
    const PanelRed rd = reds[t / (PANEL_ROWS * q4)];
    const u32 r = static_cast<u32>(t / q4) % PANEL_ROWS, q = static_cast<u32>(t % q4);
    if (rd.row0 + r >= a.M) return;
    const u32 row = a.rows[rd.row0 + r];
    const size_t slot0 = (slice * a.partials + rd.part0) * PANEL_ROWS + r;
    const float* ml = a.pml + 2u * slot0;  // partials are 16 slots apart
    const float4* p = reinterpret_cast<const float4*>(a.pacc + slot0 * Dv) + q;
    float m = ml[0];
    for (u32 i = 1; i < rd.nparts; ++i) m = fmaxf(m, ml[2u * PANEL_ROWS * i]);
    const float shift = shift_of(m);
    float ls = 0.f;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (u32 i = 0; i < rd.nparts; ++i) {
        const float f = exp2_hw((ml[2u * PANEL_ROWS * i] - shift) * a.c);
        const float4 x = p[static_cast<size_t>(i) * PANEL_ROWS * q4];
        const float fl = f * ml[2u * PANEL_ROWS * i + 1u], fx = f * x.x, fy = f * x.y, fz = f * x.z, fw = f * x.w;
        ls = i ? ls + fl : fl;
        s.x = i ? s.x + fx : fx;
        s.y = i ? s.y + fy : fy;
        s.z = i ? s.z + fz : fz;
        s.w = i ? s.w + fw : fw;
    }
    const float inv = inverse_of(ls) * a.vscale;  // (vscale 1 but for e4m3 K / V: an exact product)
    reinterpret_cast<float4*>(O + static_cast<size_t>(row) * a.O.row)[q] = make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv);
    if (q == 0 && a.lse) a.lse[slice * a.M + row] = m * a.scale + logf(ls);
}

template <int DT, int D>
PanelFn pick_dv(u32 Dv) {
    switch (Dv) {
        case 32: return k_attention_panels<DT, D, 32>;
        case 64: return k_attention_panels<DT, D, 64>;
        case 128: return k_attention_panels<DT, D, 128>;
        case 256: return k_attention_panels<DT, D, 256>;
        default: return nullptr;
    }
}

template <int DT>
PanelFn pick_d(u32 D, u32 Dv) {
    switch (D) {
        case 32: return pick_dv<DT, 32>(Dv);
        case 64: return pick_dv<DT, 64>(Dv);
        case 128: return pick_dv<DT, 128>(Dv);
        case 256: return pick_dv<DT, 256>(Dv);
        default: return nullptr;
    }
}

size_t panels_scratch_floats(const Plan& p, u32 Dv, u32 slices) {
    return attn_sat_mul(attn_sat_mul(slices, p.panel_rows.partials, PANEL_ROWS), Dv + 2u);
}

bool panels_ready(const Plan& p, u32 Dv, u32 slices) {
    return p.panel_rows.built && p.attention_panels.scratch.size() >= panels_scratch_floats(p, Dv, slices);
}

// build the lists (once, attn_panels_build_lists) and size the per-slice scratch for (Dv, slices): it
// grows and never shrinks; layout_mu held. Synchronous on the plan's stream.
int build_panels(const Plan& p, u32 Dv, u32 slices, const char* who) {
    BSMR_CHECK(attn_panels_build_lists(p, who));
    return p.attention_panels.scratch.grow(panels_scratch_floats(p, Dv, slices));
}

// the biased form: the lists and scratch above and the rows side's entry positions (the one copy in
// Plan::spmm_panels[0], spmm_panels_build_positions; no scratch of the panel SpMM)
bool panels_bias_ready(const Plan& p, u32 Dv, u32 slices) { return panels_ready(p, Dv, slices) && p.spmm_panels[0].built; }

int build_panels_bias(const Plan& p, u32 Dv, u32 slices, const char* who) {
    BSMR_CHECK(build_panels(p, Dv, slices, who));
    return spmm_panels_build_positions(p, 1, who);
}

// the 16-bit form's kernel; the dims are validated
PanelFn panels_kernel(u32 D, u32 Dv, int dtype) { return dtype == BSMR_F16 ? pick_d<BSMR_F16>(D, Dv) : pick_d<BSMR_BF16>(D, Dv); }

}  // namespace

int panel_validate_dims(const char* who, u32 D, u32 Dv, int dtype, bool with256) {
    auto dim = [&](u32 d) { return d == 32 || d == 64 || d == 128 || (with256 && d == 256); };
    if ((dtype != BSMR_F16 && dtype != BSMR_BF16) || !dim(D) || !dim(Dv)) {
        set_error(std::string(who) + ": dtype must be BSMR_F16 or BSMR_BF16 and D and Dv each one of 32, 64, 128" +
                  (with256 ? ", 256" : ""));
        return BSMR_ERR_UNSUPPORTED;
    }
    return BSMR_OK;
}

int panel_prepare_args(const char* who, const bsmr_plan* plan, u32 D, u32 Dv, u32 slices, bool with256) {
    if (!plan) {
        set_error(std::string(who) + ": null plan");
        return BSMR_ERR_INVALID;
    }
    BSMR_CHECK(attn_check_slices(who, slices));
    return panel_validate_dims(who, D, Dv, BSMR_F16, with256);
}

int attn_panels_check_dense(const char* who, const char* names, const bsmr_plan* plan, const void* dQ, const void* dK,
                            const void* dV, const void* dO, const float* dLse) {
    if (!plan) {
        set_error(std::string(who) + ": null plan");
        return BSMR_ERR_INVALID;
    }
    if (!dQ || !dK || !dV || !dO) {
        set_error(std::string(who) + ": null device pointer");
        return BSMR_ERR_INVALID;
    }
    if (!attn_aligned16(dQ) || !attn_aligned16(dK) || !attn_aligned16(dV) || !attn_aligned16(dO) ||
        (reinterpret_cast<uintptr_t>(dLse) & 3u)) {
        set_error(std::string(who) + ": " + names + " must be 16-byte aligned");
        return BSMR_ERR_INVALID;
    }
    return BSMR_OK;
}

int attn_panels_check_heads(const char* who, const bsmr_plan* plan, const float* dLse) {
    if (!plan) {
        set_error(std::string(who) + ": null plan");
        return BSMR_ERR_INVALID;
    }
    if (reinterpret_cast<uintptr_t>(dLse) & 3u) {
        set_error(std::string(who) + ": dLse must be 4-byte aligned");
        return BSMR_ERR_INVALID;
    }
    return BSMR_OK;
}

int attn_panels_launch(const char* who, const char* prep, const bsmr_plan* plan, PanelFn fn, u32 batches, u32 heads,
                       const bsmr_attention_operand& Q, const bsmr_attention_operand& K, const bsmr_attention_operand& V,
                       u32 kvBytes, u32 D, u32 Dv, int dtype, float scale, float c, float vscale,
                       const bsmr_attention_operand& O, float* dLse, void* stream, const PanelBiasIn* bias) {
    const Plan& p = plan->p;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const Plan::PanelListState& L = p.panel_rows;
    const u32 slices = batches * heads;  // (both at most 65535)
    PanelArgs a{};
    const PanelRed* reds = nullptr;
    u32 nReds = 0;
    {
        std::lock_guard<std::mutex> g(p.layout_mu);
        BSMR_CHECK(panel_build_missing(
            LaunchSite{s, who, prep, D, dtype}, [&] { return bias ? panels_bias_ready(p, Dv, slices) : panels_ready(p, Dv, slices); },
            [&] {
                return std::string("the panel lists") + (bias ? ", the entry positions" : "") + " (or their scratch for Dv = " +
                       std::to_string(Dv) + panel_slices_clause(slices) + ")";
            },
            [&] { return bias ? build_panels_bias(p, Dv, slices, prep) : build_panels(p, Dv, slices, prep); }));
        a.items = L.items.data();
        a.steps = L.steps.data();
        a.rows = L.rows.data();
        a.nItems = L.nItems;
        a.partials = L.partials;
        a.pacc = p.attention_panels.scratch.data();
        reds = L.reds.data();
        nReds = L.nReds;
        if (bias) {
            a.base = p.spmm_panels[0].base.data();
            a.pos = p.spmm_panels[0].pos.data();
        }
    }
    if (bias) {
        a.bias = bias->bias;
        a.biasStride = bias->stride;
        a.xscale = bias->scale;
    }
    a.pml = a.pacc ? a.pacc + static_cast<size_t>(slices) * a.partials * PANEL_ROWS * Dv : nullptr;
    a.Q = attn_op_bytes(&Q, batches, heads, p.M, 2u);
    a.K = attn_op_bytes(&K, batches, heads, p.N, kvBytes);
    a.V = attn_op_bytes(&V, batches, heads, p.N, kvBytes);
    a.O = attn_op_bytes(&O, batches, heads, p.M, 4u);
    a.lse = dLse;
    a.heads = heads;
    a.M = p.M;
    a.c = c;
    a.scale = scale;
    a.vscale = vscale;
    const dim3 outer(1, heads, batches);
    return panel_launch(s, fn, a, a.nItems, outer, k_attention_panels_reduce, reds, nReds, Dv / 4u, outer, Dv);
}

int panel_lists_upload(const Plan& p, Plan::PanelListState& S, int st, const std::string& err, const PanelLists& L,
                       const char* who) {
    const hipStream_t s = p.stream;
    if (st) {
        set_error(std::string(who) + ": " + err);
        return st == 2 ? BSMR_ERR_UNSUPPORTED : BSMR_ERR_INVALID;  // 2: past the lists' capacity
    }
    if (L.nItems > (1ull << 31)) {
        set_error(std::string(who) + ": more than 2^31 items");
        return BSMR_ERR_UNSUPPORTED;
    }
    BSMR_CHECK(S.rows.upload(L.rows.data(), L.rows.size(), s));
    BSMR_CHECK(S.steps.upload(L.steps.data(), L.steps.size(), s));
    BSMR_CHECK(S.items.upload(L.items.data(), L.items.size(), s));
    BSMR_CHECK(S.reds.upload(L.reds.data(), L.reds.size(), s));
    BSMR_HIP(hipStreamSynchronize(s));
    S.nItems = static_cast<u32>(L.nItems);
    S.nSteps = static_cast<u32>(L.nSteps);
    S.nReds = static_cast<u32>(L.reds.size());
    S.panels = L.panels;
    S.splitPanels = L.splitPanels;
    S.partials = L.partials;
    S.built = true;
    return BSMR_OK;
}

int attn_panels_build_lists(const Plan& p, const char* who) {
    if (p.panel_rows.built) return BSMR_OK;
    const hipStream_t s = p.stream;
    std::vector<u32> hrp, hci, hrows;
    BSMR_CHECK(p.rowptr.download(hrp, s));
    BSMR_CHECK(p.colidx.download(hci, s));
    BSMR_CHECK(p.rows.download(hrows, s));
    hrows.resize(std::min<size_t>(hrows.size(), p.R));
    PanelLists L;
    std::string err;
    // (the rows the plan's order does not name, its empty ones, get trailing panels of 0 steps; the
    // lists would compute them from their entries all the same)
    const int st = attention_panel_lists(p.M, p.N, hrp.data(), hci.data(), hrows.data(), static_cast<u32>(hrows.size()), L, err);
    return panel_lists_upload(p, p.panel_rows, st, err, L, who);
}

}  // namespace bsmr

using namespace bsmr;

extern "C" int bsmr_attention_panels(const bsmr_plan* plan, const void* dQ, const void* dK, const void* dV, uint32_t D,
                                     uint32_t Dv, int dtype, float scale, float* dO, float* dLse, void* stream) {
    const char* who = "bsmr_attention_panels";
    BSMR_CHECK(attn_panels_check_dense(who, "dQ, dK, dV and dO", plan, dQ, dK, dV, dO, dLse));
    float c;
    BSMR_CHECK(attn_validate_scale(who, scale, &c));
    BSMR_CHECK(panel_validate_dims(who, D, Dv, dtype, true));
    const Plan& p = plan->p;
    return attn_panels_launch(who, "bsmr_plan_prepare_attention_panels", plan, panels_kernel(D, Dv, dtype), 1, 1,
                              attention_dense_operand(dQ, 1, p.M, D), attention_dense_operand(dK, 1, p.N, D),
                              attention_dense_operand(dV, 1, p.N, Dv), 2u, D, Dv, dtype, scale, c, 1.0f,
                              attention_dense_operand(dO, 1, p.M, Dv), dLse, stream);
}

extern "C" int bsmr_attention_panels_heads(const bsmr_plan* plan, uint32_t batches, uint32_t heads,
                                           const bsmr_attention_operand* Q, const bsmr_attention_operand* K,
                                           const bsmr_attention_operand* V, uint32_t D, uint32_t Dv, int dtype, float scale,
                                           const bsmr_attention_operand* O, float* dLse, void* stream) {
    const char* who = "bsmr_attention_panels_heads";
    BSMR_CHECK(attn_panels_check_heads(who, plan, dLse));
    float c;
    BSMR_CHECK(attn_validate_scale(who, scale, &c));
    BSMR_CHECK(panel_validate_dims(who, D, Dv, dtype, true));
    const Plan& p = plan->p;
    BSMR_CHECK(attn_check_operand(who, "Q", Q, batches, heads, p.M, D, 2u, false));
    BSMR_CHECK(attn_check_operand(who, "K", K, batches, heads, p.N, D, 2u, false));
    BSMR_CHECK(attn_check_operand(who, "V", V, batches, heads, p.N, Dv, 2u, false));
    BSMR_CHECK(attn_check_operand(who, "O", O, batches, heads, p.M, Dv, 4u, true));
    return attn_panels_launch(who, "bsmr_plan_prepare_attention_panels_heads", plan, panels_kernel(D, Dv, dtype), batches,
                              heads, *Q, *K, *V, 2u, D, Dv, dtype, scale, c, 1.0f, *O, dLse, stream);
}

extern "C" int bsmr_plan_prepare_attention_panels_heads(const bsmr_plan* plan, uint32_t D, uint32_t Dv, uint32_t slices) {
    const char* who = "bsmr_plan_prepare_attention_panels_heads";
    BSMR_CHECK(panel_prepare_args(who, plan, D, Dv, slices, true));
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return build_panels(plan->p, Dv, slices, who);
}

extern "C" int bsmr_plan_prepare_attention_panels(const bsmr_plan* plan, uint32_t D, uint32_t Dv) {
    const char* who = "bsmr_plan_prepare_attention_panels";
    BSMR_CHECK(panel_prepare_args(who, plan, D, Dv, 1, true));
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return build_panels(plan->p, Dv, 1, who);
}

extern "C" int bsmr_plan_attention_panels_heads_prepared(const bsmr_plan* plan, uint32_t D, uint32_t Dv, uint32_t slices) {
    if (panel_prepare_args("bsmr_plan_attention_panels_heads_prepared", plan, D, Dv, slices, true) != BSMR_OK) return 0;
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return panels_ready(plan->p, Dv, slices) ? 1 : 0;
}

extern "C" int bsmr_plan_attention_panels_prepared(const bsmr_plan* plan, uint32_t D, uint32_t Dv) {
    return bsmr_plan_attention_panels_heads_prepared(plan, D, Dv, 1);
}

// a biased prepare's (D, Dv): the forms attention_panels_bias.hip builds
static int bias_prepare_args(const char* who, const bsmr_plan* plan, uint32_t D, uint32_t Dv, uint32_t slices) {
    BSMR_CHECK(panel_prepare_args(who, plan, D, Dv, slices, true));
    if (!panels_bias_kernel(D, Dv, BSMR_F16)) {
        set_error(std::string(who) + ": the biased form of D = " + std::to_string(D) + ", Dv = " + std::to_string(Dv) + " is not built");
        return BSMR_ERR_UNSUPPORTED;
    }
    return BSMR_OK;
}

extern "C" int bsmr_plan_prepare_attention_panels_bias_heads(const bsmr_plan* plan, uint32_t D, uint32_t Dv, uint32_t slices) {
    const char* who = "bsmr_plan_prepare_attention_panels_bias_heads";
    BSMR_CHECK(bias_prepare_args(who, plan, D, Dv, slices));
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return build_panels_bias(plan->p, Dv, slices, who);
}

extern "C" int bsmr_plan_prepare_attention_panels_bias(const bsmr_plan* plan, uint32_t D, uint32_t Dv) {
    const char* who = "bsmr_plan_prepare_attention_panels_bias";
    BSMR_CHECK(bias_prepare_args(who, plan, D, Dv, 1));
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return build_panels_bias(plan->p, Dv, 1, who);
}

extern "C" int bsmr_plan_attention_panels_bias_heads_prepared(const bsmr_plan* plan, uint32_t D, uint32_t Dv, uint32_t slices) {
    if (bias_prepare_args("bsmr_plan_attention_panels_bias_heads_prepared", plan, D, Dv, slices) != BSMR_OK) return 0;
    std::lock_guard<std::mutex> g(plan->p.layout_mu);
    return panels_bias_ready(plan->p, Dv, slices) ? 1 : 0;
}

extern "C" int bsmr_plan_attention_panels_bias_prepared(const bsmr_plan* plan, uint32_t D, uint32_t Dv) {
    return bsmr_plan_attention_panels_bias_heads_prepared(plan, D, Dv, 1);
}

extern "C" int bsmr_plan_attention_panels_stats(const bsmr_plan* plan, bsmr_attention_panels_stats* out) {
    if (!plan || !out) {
        set_error("bsmr_plan_attention_panels_stats: null argument");
        return BSMR_ERR_INVALID;
    }
    const Plan& p = plan->p;
    std::lock_guard<std::mutex> g(p.layout_mu);
    *out = bsmr_attention_panels_stats{};
    out->step_cols = PANEL_STEP_COLS;
    out->item_steps = PANEL_ITEM_STEPS;
    if (p.panel_rows.built)
        panel_list_stats(p.panel_rows, p.nnz, out->panels, out->items, out->steps, out->split_panels, out->partials,
                         out->fill_permille);
    return BSMR_OK;
}
