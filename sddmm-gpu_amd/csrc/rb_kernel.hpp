// rb_kernel.hpp — the row-block SDDMM kernels' device code: the launch argument
// record RbArgs, the LDS image and its staging by LDS-DMA, dense tiles and column-run pieces on the
// image, the steps of a work item as functions, the two kernels that run them (k_sddmm_rb: one
// item, full or lite; k_sddmm_rb_pair: two items through rb_item) and pick_rb, which maps a
// launch's form to an instantiation. Included by sddmm.hip only, inside
// whose translation unit (and anonymous namespace) the kernels live; launch_rb there fills RbArgs
// and launches what pick_rb returns.
#pragma once

#include <type_traits>

#include "common.hpp"
#include "plan.hpp"
#include "sddmm_device.hpp"

namespace bsmr {
namespace {

// ==========================================================================================
// Row-block launch (rows of RBY = 256 or 512 bytes: fp32 K = 64/128, fp16/bf16 K = 128/256): one
// workgroup per item {row block rb, tiles [t0, t1), residual pieces [p0, p1)} (layout:
// Plan::build_rowblock_layout). The A rows of the RB reordered positions of rb are staged in LDS
// once (<= 144 KiB); dense tiles take their MFMA A operand and residual entries their A pieces
// from LDS, so the only gathered operand is B, read once per column run (entries are sorted by
// (row block, column)).
//
// Residual entries: G = 4 lanes per entry (16 row-groups per wave), so the per-entry bookkeeping
// (metadata broadcast, addresses, store) is shared by 16 entries per wave instruction; each lane
// owns NC = RBY/64 16-byte chunks 4t + s of the row (packed FMA for fp32, v_dot2 for fp16/bf16,
// fp32 accumulation) and the quad reduces with two DPP adds.
// LDS image: row lr at lr * RBY bytes (unpadded); chunk c of row lr sits at
// (c & ~3) | ((c & 3) ^ (lr & 3)). Lane (row-group j, sub s) visits its chunks in the rotated
// order t = (f + j) mod NC, so in every ds_read_b128 lane group ({0-3,12-15,20-27},
// {4-11,16-19,28-31}, +32 = row-groups {0,3,5,6}, {1,2,4,7}, ...) the four row-groups read four
// different 64-byte quads: conflict-free for any rows (the XOR only permutes inside a quad).
// Dense tiles read chunk 16w + 4g + j of the 16 tile rows: the XOR spreads rows 0-3 (2-way).
// ==========================================================================================
struct RbArgs {
    const char* A;  // row-major M x K elements of the dtype
    const char* B;  // N rows of K elements (B column-major)
    float* P;
    const u32* rows;
    u32 R, N, RB;  // R: rows at or past this reordered position are not staged (range end)
    u32 qbase;     // reordered position of row block 0 (16 * first panel of the range)
    u32 row0;      // row staged for positions outside the block (its unused image tail): a row
                   // the launch's A holds (0, or 16 * first panel for a shard-local A)
    const uint4* items;     // {row block, tile begin, tile end, piece begin}
    const u32* itemEnd;     // piece end
    const uint2* pieces;    // {first entry, column | (length - 1) << 22}
    const u32* meta;        // local row << 22 | column
    const u32* out;
    const uint4* tilePanel;  // dense work items: .x = panel of the tile
    const u32* tileIds;      // the layout's kept tiles: item tile ranges index this list
    const u32* denseCols;
    const u32* blockValues;
    u32 mode;  // 1 = dense tiles, 2 = residual, 3 = both
    // staged output (Plan::RowBlockLayout::outLds): != 0 = byte offset of the item's result slots
    // in LDS; the entry metadata's low bits are then the slot, and the workgroup writes the slots
    // to P[sortedPos[itemEnt.x + t]] at the end
    u32 outLds;
    u32 outPacked;  // 1: no out array, the metadata's low 22 bits are the CSR position
    u32 stageNt;  // 1: stage the A rows with the nt policy (Knobs::stage_nt)
    u32 lateB;    // 1: phase-0 B columns / metadata loaded after the staging barrier (late_b)
    u32 stageBlocks;  // 1 KiB LDS-DMA blocks that hold the image (RB * RBY / 1024); the rest of
                      // the workgroup's LDS is not staged
    const u32* sortedPos;
    const uint2* itemEnt;
    // staged output by runs (RowBlockLayout::outRuns; else null): {position, slot | len << 16}, len <= 64
    // per run of consecutive CSR positions, {first run, runs} per item
    const uint2* runs;
    const uint2* itemRuns;
    u32 pairs;  // 1: each workgroup runs list positions 2j and 2j + 1 of its XCD (see k_sddmm_rb_pair)
    unsigned long long* trace;  // BSMR_DIAG & 32 timeline (see trace_wave)
    u32 diag;                   // profiling ablations (BSMR_DIAG); always 0 in normal use
    unsigned long long bA, bB, bP;  // batched launch: A, B byte strides, P element stride
};

// KiB of LDS a row-block workgroup is launched with (launch_select.cpp rb_form, ldsBytes): the
// image, the staged-output slots and, in the last word, the piece-batch counter
constexpr u32 rb_lds_kib(const int NT) { return NT == 1024 ? 160u : 80u; }

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 b16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 b16x8 __attribute__((ext_vector_type(8)));

// physical 16-byte chunk of logical chunk c of image row lr. fp16/bf16 images swizzle inside each
// 64-byte quad so the MFMA tile reads (4 chunk-consecutive rows per lane group) spread over the
// banks; fp32 images are plain (no tiles on the fp32 row-block path; the residual reads are
// conflict-free by the rotation alone), which saves the swizzle arithmetic per entry.
template <int DT>
__device__ __forceinline__ u32 lds_chunk(u32 lr, u32 c) {
    if constexpr (DT == 0)
        return c;
    else
        return (c & ~3u) | ((c & 3u) ^ (lr & 3u));
}

__device__ __forceinline__ f32x4 ld16(const char* p) { return *reinterpret_cast<const f32x4*>(p); }

// one staging LDS-DMA wave-instruction: 16 bytes per lane from g to LDS at l + 16 * lane (l
// wave-uniform). Inline asm, so the compiler's wait-count pass does not track it: around the
// builtin, a branch (skipping the blocks past the image) made the compiler wait (vmcnt(0)) for
// every LDS-DMA before issuing the next. The kernels order these by their explicit
// s_waitcnt vmcnt(0) + barrier before the image is read. AUX 2: the nt cache policy.
// LDS byte address of a pointer into the workgroup's LDS
__device__ __forceinline__ u32 lds_addr(const char* l) {
    return __builtin_amdgcn_readfirstlane(static_cast<u32>(
        reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) const char*)l)));
}
template <int AUX>
__device__ __forceinline__ void rb_dma16(const char* g, const u32 m0) {
    if constexpr (AUX == 2)
        asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off nt" ::"v"(g), "s"(m0)
                     : "memory", "m0");
    else
        asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(m0)
                     : "memory", "m0");
}

// value of lane I of the quad in every lane of the quad
template <int I>
__device__ __forceinline__ u32 quad_bcast(u32 v) {
    return static_cast<u32>(
        __builtin_amdgcn_update_dpp(0, static_cast<int>(v), I * 0x55, 0xF, 0xF, false));
}

// acc += a . b over one 16-byte chunk (DT 0: 4 fp32, packed FMA; 1: 8 fp16, 2: 8 bf16, v_dot2)
template <int DT>
__device__ __forceinline__ void chunk_dot(const f32x4 a, const f32x4 b, f32x2& acc0, f32x2& acc1) {
    if constexpr (DT == 0) {
        acc0 = __builtin_elementwise_fma(f32x2{a.x, a.y}, f32x2{b.x, b.y}, acc0);
        acc1 = __builtin_elementwise_fma(f32x2{a.z, a.w}, f32x2{b.z, b.w}, acc1);
    } else if constexpr (DT == 1) {
        // whole-vector bit casts + swizzles: __builtin_bit_cast of a vector ELEMENT miscompiles
        // here (hipcc 7.2 reads element 0 for every index)
        const h16x8 ha = __builtin_bit_cast(h16x8, a), hb = __builtin_bit_cast(h16x8, b);
        acc0.x = __builtin_amdgcn_fdot2(ha.s01, hb.s01, acc0.x, false);
        acc0.y = __builtin_amdgcn_fdot2(ha.s23, hb.s23, acc0.y, false);
        acc1.x = __builtin_amdgcn_fdot2(ha.s45, hb.s45, acc1.x, false);
        acc1.y = __builtin_amdgcn_fdot2(ha.s67, hb.s67, acc1.y, false);
    } else {
        const b16x8 ha = __builtin_bit_cast(b16x8, a), hb = __builtin_bit_cast(b16x8, b);
        acc0.x = __builtin_amdgcn_fdot2_f32_bf16(ha.s01, hb.s01, acc0.x, false);
        acc0.y = __builtin_amdgcn_fdot2_f32_bf16(ha.s23, hb.s23, acc0.y, false);
        acc1.x = __builtin_amdgcn_fdot2_f32_bf16(ha.s45, hb.s45, acc1.x, false);
        acc1.y = __builtin_amdgcn_fdot2_f32_bf16(ha.s67, hb.s67, acc1.y, false);
    }
}

// acc += the MFMA of one 16-byte A chunk and B chunk per lane (DT 0: four 16x16x4 f32 steps;
// 1/2: one 16x16x32 f16/bf16 step), lane layout of dense_tile (one k-block per lane group)
template <int DT>
__device__ __forceinline__ f32x4 chunk_mfma(const f32x4 a, const f32x4 b, f32x4 acc) {
    if constexpr (DT == 0) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    } else if constexpr (DT == 1) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, a),
                                                      __builtin_bit_cast(h16x8, b), acc, 0, 0, 0);
    } else {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b16x8, a),
                                                       __builtin_bit_cast(b16x8, b), acc, 0, 0, 0);
    }
}

// lanes per residual entry for a row size: 4 up to 512-byte rows, 8 for 1 KiB, 16 for 2 KiB rows;
// every lane then owns NC = RBY / (16 * G) <= 8 chunks of the row
template <int RBY>
struct RowGeom {
    static constexpr u32 G = RBY >= 2048 ? 16 : RBY >= 1024 ? 8 : 4;
    static constexpr u32 NC = RBY / (16 * G);
    static constexpr u32 NB = (RB_PIECE_MAX + G - 1) / G;  // metadata batches per piece
    // distinct chunk-group rotations the residual reads need: a ds_read_b128 lane group
    // (MI355X_MICROARCH.md §LDS: {0-3,12-15,20-27}, {4-11,16-19,28-31}, +32) holds 4 row-groups
    // of 4 lanes whose 64-byte reads must fill the 256-byte bank row (rotations j mod 4 differ
    // inside each), halves of 4 8-lane groups (j mod 2 moves them by 128 bytes), or one 16-lane
    // group that already spans it. Reads f <= NC - RR never wrap, so they address one base
    // register with immediate offsets.
    static constexpr u32 RR = (G == 4 ? 4u : G == 8 ? 2u : 1u) < NC ? (G == 4 ? 4u : G == 8 ? 2u : 1u) : NC;
};

// value of lane I of the G-lane group in every lane of the group
template <int G, int I>
__device__ __forceinline__ u32 group_bcast(u32 v) {
    if constexpr (G == 4)
        return quad_bcast<I>(v);
    else if constexpr (G == 8)  // ds_swizzle bit mode: and 0x18 (the group), or I
        return static_cast<u32>(__builtin_amdgcn_ds_swizzle(static_cast<int>(v), 0x18 | (I << 5)));
    else  // a whole DPP row
        return row_bcast<I>(v);
}

// dense tile on the LDS image: load() gathers the tile's metadata and B operand (no LDS, so a
// wave can issue it before the staging barrier), run() reads the A rows from LDS, runs the MFMAs
// and scatters the 256 outputs. Lane group g takes chunk 16w + 4g + j at k-step 4w + j (any
// k-permutation shared by A and B is valid), so the XOR of the LDS image spreads it. Rows of
// 1 KiB (16 chunks per lane) are processed in two halves of 8 chunks.
template <int DT, int RBY>
struct DenseTileLds {
    static constexpr int NK = RBY / 64;          // 16-byte chunks per lane
    static constexpr int CH = NK > 8 ? 8 : NK;   // chunks held in registers at once
    u32 lr, c, idx[4];
    __device__ __forceinline__ static u32 chunk(int kk, u32 g) {
        if constexpr (NK >= 4)
            return 16 * (kk >> 2) + 4 * g + (kk & 3);
        else  // 128-byte rows: k-step kk covers chunks kk, NK + kk, 2 NK + kk, 3 NK + kk
            return NK * g + kk;
    }
    __device__ __forceinline__ void meta(const RbArgs& a, const u32 tile, const u32 q0) {
        const u32 l = __lane_id(), rr = l & 15, g = l >> 4;
        const u32 p = a.tilePanel[tile].x;
        c = a.denseCols[tile * 16 + rr];
        const u32* bvals = a.blockValues + static_cast<size_t>(tile) * 256 + 64 * g + rr;
#pragma unroll
        for (int r = 0; r < 4; ++r) idx[r] = bvals[16 * r];
        lr = p * 16 - q0 + rr;
    }
    // B chunks [k0, k0 + CH)
    __device__ __forceinline__ void loadB(const RbArgs& a, const int k0, f32x4 (&bv)[CH]) const {
        const u32 g = __lane_id() >> 4;
        const bool cvalid = c < a.N;
        // BSMR_DIAG & 8388608 (ablation only): every tile reads B column 0, so its gathers hit L2
        const char* bcol = a.B + static_cast<size_t>(cvalid && !(a.diag & 8388608u) ? c : 0) * RBY;
#pragma unroll
        for (int kk = 0; kk < CH; ++kk)
            bv[kk] = cvalid ? ld16(bcol + 16 * chunk(k0 + kk, g)) : f32x4{0, 0, 0, 0};
    }
    __device__ __forceinline__ void load(const RbArgs& a, const u32 tile, const u32 q0,
                                         f32x4 (&bv)[CH]) {
        meta(a, tile, q0);
        loadB(a, 0, bv);
    }
    // bv: the first CH chunks (from load); later halves are loaded here
    __device__ __forceinline__ void run(const RbArgs& a, const char* As, f32x4 (&bv)[CH]) const {
        const u32 g = __lane_id() >> 4;
        const char* arow = As + lr * RBY;
        f32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
#pragma unroll
        for (int k0 = 0; k0 < NK; k0 += CH) {
            if (k0) loadB(a, k0, bv);
#pragma unroll
            for (int kk = 0; kk < CH; ++kk) {
                const f32x4 av = ld16(arow + 16 * lds_chunk<DT>(lr, chunk(k0 + kk, g)));
                f32x4& acc = (kk & 1) ? acc1 : acc0;
                acc = chunk_mfma<DT>(av, bv[kk], acc);
            }
        }
        const f32x4 acc = acc0 + acc1;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (idx[r] != NULLV) a.P[idx[r]] = acc[r];
    }
};

// B pieces of the group's column (lane s: chunks G * ((f + j) mod NC) + s, f < NC)
template <int RBY>
__device__ __forceinline__ void load_bcol(const RbArgs& a, const u32 col, const u32 sub,
                                          const u32 (&rot)[RowGeom<RBY>::NC],
                                          f32x4 (&bv)[RowGeom<RBY>::NC]) {
    // B < 4 GiB on this path (launch_select.cpp); BSMR_DIAG & 64 (ablation only): every piece reads
    // column 0, so the B gathers hit L2
    const u32 bb = ((a.diag & 64) ? 0u : col) * RBY + 16 * sub;
#pragma unroll
    for (u32 f = 0; f < RowGeom<RBY>::NC; ++f)
        bv[f] = f + RowGeom<RBY>::RR <= RowGeom<RBY>::NC
                    ? ld16(a.B + (bb + rot[0]) + 16 * RowGeom<RBY>::G * f)  // no wrap: immediate
                    : ld16(a.B + (bb + rot[f]));
}

// a column-run piece of a row-group: entries [first, first + len), len <= RB_PIECE_MAX, all
// in one column. Lane s of the group holds the metadata of entries first + G*k + s.
template <int RBY>
struct Piece {
    u32 first, len, col;
    u32 mm[RowGeom<RBY>::NB], mo[RowGeom<RBY>::NB];
};

// the piece descriptor (first entry, column, length)
template <int RBY>
__device__ __forceinline__ void load_piece_desc(const RbArgs& a, const u32 pi, Piece<RBY>& pc) {
    const uint2 d = a.pieces[pi];
    pc.first = d.x;
    pc.len = (d.y >> 22) + 1;
    pc.col = d.y & 0x3FFFFFu;
}

// the piece's B column and its entries' metadata (after load_piece_desc)
template <int RBY>
__device__ __forceinline__ void load_piece_body(const RbArgs& a, const u32 sub,
                                                const u32 (&rot)[RowGeom<RBY>::NC],
                                                f32x4 (&bv)[RowGeom<RBY>::NC], Piece<RBY>& pc) {
    constexpr u32 G = RowGeom<RBY>::G;
    load_bcol<RBY>(a, pc.col, sub, rot, bv);
#pragma unroll
    for (u32 k = 0; k < RowGeom<RBY>::NB; ++k) {
        const u32 e = G * k + sub;
        pc.mm[k] = e < pc.len ? a.meta[pc.first + e] : 0u;
        // staged output: the slot is the metadata's low bits, taken where the result is stored
        // (deriving it here made the prologue wait for this load, and so for the B column
        // before it, ahead of the staging)
        pc.mo[k] = !a.outLds && !a.outPacked && e < pc.len ? a.out[pc.first + e] : 0u;
    }
}

template <int RBY>
__device__ __forceinline__ void load_piece(const RbArgs& a, const u32 pi, const u32 sub,
                                           const u32 (&rot)[RowGeom<RBY>::NC],
                                           f32x4 (&bv)[RowGeom<RBY>::NC], Piece<RBY>& pc) {
    load_piece_desc<RBY>(a, pi, pc);
    load_piece_body<RBY>(a, sub, rot, bv, pc);
}

// Step i of a batch of G computes entry G*k + i in all G lanes; lane i keeps it, so a batch ends
// in one store instruction for G entries per group (64 outputs per full wave).
template <int DT, int RBY>
__device__ __forceinline__ void residual_piece(const RbArgs& a, const char* As,
                                               const Piece<RBY>& pc, const u32 sub,
                                               const u32 (&rot)[RowGeom<RBY>::NC],
                                               const f32x4 (&bv)[RowGeom<RBY>::NC]) {
    constexpr u32 G = RowGeom<RBY>::G, NC = RowGeom<RBY>::NC;
#pragma unroll
    for (u32 k = 0; k < RowGeom<RBY>::NB; ++k) {
        if (G * k >= pc.len) break;
        const u32 nb = min(G, pc.len - G * k);
        // fp32 images are unswizzled: broadcast the image row offset lr * RBY itself, computed
        // once per batch by the lane that owns the entry, instead of shifting m in every step
        const u32 mk = DT == 0 ? (pc.mm[k] >> 22) * RBY : pc.mm[k];
        float res = 0.f;
#pragma unroll
        for (int i = 0; i < static_cast<int>(G); ++i) {
            if (static_cast<u32>(i) >= nb) break;
            u32 m;
            switch (i) {
#define BSMR_C(I) \
    case I: m = group_bcast<G, (I < G ? I : 0)>(mk); break;
                BSMR_C(0) BSMR_C(1) BSMR_C(2) BSMR_C(3) BSMR_C(4) BSMR_C(5) BSMR_C(6) BSMR_C(7)
                BSMR_C(8) BSMR_C(9) BSMR_C(10) BSMR_C(11) BSMR_C(12) BSMR_C(13) BSMR_C(14)
#undef BSMR_C
                default: m = group_bcast<G, G - 1>(mk); break;
            }
            u32 ab;  // + rot[f]: chunk G t + sub
            if constexpr (DT == 0) {
                ab = m + 16 * sub;
            } else {
                const u32 lr = m >> 22;
                ab = lr * RBY + 16 * lds_chunk<DT>(lr, sub);
            }
            const char* arot = As + (ab + rot[0]);                   // no wrap before f = NC - RR
            f32x2 acc0 = {0.f, 0.f}, acc1 = {0.f, 0.f};
            constexpr u32 H = NC > 4 ? NC / 2 : NC;  // LDS reads in flight per half
#pragma unroll
            for (u32 h = 0; h < NC; h += H) {
                f32x4 av[H];
#pragma unroll
                for (u32 f = 0; f < H; ++f)
                    av[f] = h + f + RowGeom<RBY>::RR <= NC ? ld16(arot + 16 * G * (h + f))
                                                           : ld16(As + (ab + rot[h + f]));
#pragma unroll
                for (u32 f = 0; f < H; ++f) {
                    if constexpr (DT == 0)  // one packed chain: no acc0 + acc1 per entry
                        chunk_dot<DT>(av[f], bv[h + f], acc0, acc0);
                    else
                        chunk_dot<DT>(av[f], bv[h + f], acc0, acc1);
                }
            }
            f32x2 acc = acc0;
            if constexpr (DT != 0) acc += acc1;
            float sm = acc.x + acc.y;
            sm += dppf<0xB1>(sm);                         // quad_perm [1,0,3,2]
            sm += dppf<0x4E>(sm);                         // quad_perm [2,3,0,1]
            if constexpr (G >= 8) sm += dppf<0x141>(sm);   // row_half_mirror: the other quad
            if constexpr (G == 16) sm += dppf<0x140>(sm);  // row_mirror: the other half-row
            if (sub == static_cast<u32>(i)) res = sm;
        }
        if (sub < nb) {
            if (a.outLds)  // the slot: rank by CSR position inside the item
                *reinterpret_cast<float*>(const_cast<char*>(As) + a.outLds +
                                          4 * (pc.mm[k] & 0x3FFFFFu)) = res;
            else
                a.P[a.outPacked ? pc.mm[k] & 0x3FFFFFu : pc.mo[k]] = res;
        }
    }
}

// Dynamic piece batches (RowBlockLayout::dynBatches, rows of <= 512 B): batch b = the item's
// pieces [b GW, (b + 1) GW), GW = 64 / G, one per row-group of a wave. Wave w runs batch w first
// (the static phase 0), then takes the next batch from a counter in the workgroup's last LDS word
// (the layout keeps it free), so waves whose pieces were short or whose gathers were fast take
// more of an item with many pieces per row-group. The next batch's piece is loaded while the
// current one computes, as in the static phases. Returns after the wave's last batch.
constexpr u32 BATCH_CTR_BYTES = 16;  // the counter's share of the workgroup's LDS (its end)
template <int NT>
__device__ __forceinline__ u32* rb_batch_ctr(const char* As) {  // the counter: the last LDS word
    return reinterpret_cast<u32*>(const_cast<char*>(As) + rb_lds_kib(NT) * 1024u - 4u);
}
template <int DT, int RBY, int NT, typename LoadRuns>
__device__ __forceinline__ void rb_batches(const RbArgs& a, const char* As, const u32 p0, const u32 np,
                                           const u32 gr, const u32 sub, const u32 (&rot)[RowGeom<RBY>::NC],
                                           Piece<RBY>& pc, f32x4 (&pre)[RowGeom<RBY>::NC], LoadRuns&& load_runs) {
    constexpr u32 NC = RowGeom<RBY>::NC, GW = 64 / RowGeom<RBY>::G, NW = NT / 64;
    u32* const ctr = rb_batch_ctr<NT>(As);
    auto grab = [&]() -> u32 {
        u32 v = 0;
        if ((threadIdx.x & 63) == 0)
            v = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return NW + static_cast<u32>(__builtin_amdgcn_readfirstlane(static_cast<int>(v)));
    };
    Piece<RBY> pn;
    f32x4 nb[NC];
    auto fetch = [&](const u32 b) {
        const u32 pi = b * GW + gr % GW;
        pn.len = 0;
        if (pi < np) load_piece<RBY>(a, p0 + pi, sub, rot, nb, pn);
    };
    u32 bn = grab();
    if (bn * GW < np)
        fetch(bn);
    else
        load_runs();
    if (pc.len) residual_piece<DT, RBY>(a, As, pc, sub, rot, pre);
    while (bn * GW < np) {
        pc = pn;
#pragma unroll
        for (u32 f = 0; f < NC; ++f) pre[f] = nb[f];
        bn = grab();
        if (bn * GW < np)
            fetch(bn);
        else
            load_runs();
        if (pc.len) residual_piece<DT, RBY>(a, As, pc, sub, rot, pre);
    }
}

constexpr u32 NO_ITEM = 0xFFFFFFFFu;
// run values a wave holds in registers while the next item's staging is issued (pairs)
constexpr u32 PAIR_RUNS_PER_WAVE = 16;

// the staging of a row block: wave w of NW issues the 1 KiB blocks w + i NW, i < MAXB, of the
// workgroup's LDS; a block holds 64 chunks = 64 / NCH rows and starts NR rows
template <int RBY, int NT>
struct StageGeom {
    static constexpr u32 NW = NT / 64;    // waves per workgroup
    static constexpr u32 NCH = RBY / 16;  // 16-byte chunks per row
    static constexpr u32 NR = NCH >= 64 ? 1 : 64 / NCH;  // rows a block starts (<= 4)
    static constexpr u32 MAXB = rb_lds_kib(NT) / NW;
    static_assert(MAXB * NW == rb_lds_kib(NT), "whole KiB blocks");
    static constexpr bool ROWV = MAXB * NR <= 64;  // one row index per lane (else 128-byte rows)
    static constexpr u32 NSRC = ROWV ? 1 : MAXB;   // per-lane row indices of 128-byte rows
};

// the item's descriptor {row block, tile begin, tile end, piece begin} and piece end; true for a
// padding item (uniform across the workgroup)
__device__ __forceinline__ bool rb_load_item(const RbArgs& a, const u32 idx, uint4& it, u32& pend) {
    it = a.items[idx];
    // all four fields in SGPRs before the padding test: the compiler otherwise loads .x (the row
    // block) in a second, dependent round trip after the test
    it.x = __builtin_amdgcn_readfirstlane(it.x);
    it.y = __builtin_amdgcn_readfirstlane(it.y);
    it.z = __builtin_amdgcn_readfirstlane(it.z);
    it.w = __builtin_amdgcn_readfirstlane(it.w);
    pend = a.itemEnd[idx];
    return it.y == it.z && it.w == pend;
}

// staging row indices of the row block starting at reordered position q0, one per lane (rows of
// >= 256 bytes: lane l holds the row of block w + (l / NR) NW, rows l % NR of it)
template <int RBY, int NT>
__device__ __forceinline__ u32 rb_stage_rows(const RbArgs& a, const u32 q0, const u32 ws, const u32 lane) {
    using SG = StageGeom<RBY, NT>;
    const u32 i = lane / SG::NR, b = ws + i * SG::NW, lr = 64 * b / SG::NCH + lane % SG::NR, q = q0 + lr;
    return (i < SG::MAXB && lr < a.RB && q < a.R) ? a.rows[q] : a.row0;
}

// Staging a row block by LDS-DMA: each wave-instruction fills one contiguous KiB of the image
// (64 chunks of the row-major image); lane l supplies image chunk x = 64 b + l, i.e. row
// lr = x / NCH at physical chunk pc = x % NCH, read from the logical chunk lds_chunk(lr, pc)
// of A[rows[q0 + lr]] (the XOR is an involution). The row indices of the wave's blocks are
// loaded once, one per lane, and handed to the block's lanes with v_readlane + select.
// Wave w stages the image's blocks b = w + i NW < stageBlocks, back to back, by inline-asm
// LDS-DMAs (rb_dma16): around the builtin, a branch (skipping a block) or any LDS instruction
// between two LDS-DMAs made the compiler wait (vmcnt(0)) for each LDS-DMA before issuing the
// next, which serialised the staging (C2: 12.8 -> 12.0 us once removed); until round 5 every
// wave therefore staged the launch's whole LDS, the blocks past the image reading row 0.
// This function: the LDS-DMAs of one row block (rows of >= 256 bytes; rowv from rb_stage_rows): every wave
// issues its 1 KiB blocks of the image back to back. UNROLL: the unroll count of the issue loop. ws
// and lane are references, as are the scalar parameters of the functions below: the loop then sees
// the caller's own variables, as the capturing lambda it replaces did, and compiles to the same
// code; taken by value, the single-item kernels' issue loops came out differently
template <int DT, int RBY, int NT, int AUX, int UNROLL>
__device__ __forceinline__ void rb_stage_issue(const RbArgs& a, char* As, u32 rowv, const u32& ws,
                                               const u32& lane) {
    using SG = StageGeom<RBY, NT>;
    // a rolled loop: the row indices in registers before the first LDS-DMA: the compiler does not
    // count the (inline asm) DMAs, so a wait for the indices inside the loop (at its head) would
    // also wait for every DMA issued before it
    if constexpr (UNROLL < static_cast<int>(SG::MAXB)) asm volatile("" : "+v"(rowv));
    // the source chunk of lane l is the same in every block of the wave: x % NCH and
    // (x / NCH) & 3 for x = 64 (ws + i NW) + l do not depend on i (NW = 16 or 8, NCH >= 8)
    const u32 x0 = 64 * ws + lane;
    const u32 coff = 16 * lds_chunk<DT>(x0 / SG::NCH, x0 % SG::NCH);
#pragma unroll UNROLL
    for (u32 i = 0; i < SG::MAXB; ++i) {
        const u32 b = ws + i * SG::NW;
        u32 src = static_cast<u32>(__builtin_amdgcn_readlane(static_cast<int>(rowv), i * SG::NR));
#pragma unroll
        for (u32 k = 1; k < SG::NR; ++k) {
            const u32 rk = static_cast<u32>(__builtin_amdgcn_readlane(static_cast<int>(rowv), i * SG::NR + k));
            src = lane / SG::NCH == k ? rk : src;
        }
        const char* g = a.A + (static_cast<size_t>(src) * RBY + coff);
        if (b < a.stageBlocks) rb_dma16<AUX>(g, lds_addr(As) + 1024 * b);
    }
}

// the same for 128-byte rows (src: the row of the lane's own chunk, per block)
template <int DT, int RBY, int NT, int AUX>
__device__ __forceinline__ void rb_stage_issue128(const RbArgs& a, char* As,
                                                  const u32 (&src)[StageGeom<RBY, NT>::NSRC], const u32& ws,
                                                  const u32& lane) {
    using SG = StageGeom<RBY, NT>;
    const u32 x0 = 64 * ws + lane;  // (the lane's source chunk: see rb_stage_issue)
    const u32 coff = 16 * lds_chunk<DT>(x0 / SG::NCH, x0 % SG::NCH);
#pragma unroll
    for (u32 i = 0; i < SG::MAXB; ++i) {
        const u32 b = ws + i * SG::NW;
        const char* g = a.A + (static_cast<size_t>(src[i]) * RBY + coff);
        if (b < a.stageBlocks) rb_dma16<AUX>(g, lds_addr(As) + 1024 * b);
    }
}

// staged output by per-result positions (ie: the item's {first entry, entries}): eight position
// loads in flight per lane before their stores: a loop of dependent load -> store pairs exposed
// one L2 latency per 1024 results (C4 x0.5: 1.135 -> 1.082 ms). Issuing the first batch before
// the barrier measured slower (1.109 ms)
template <int NT>
__device__ __forceinline__ void store_sorted(const RbArgs& a, const float* const& res, const uint2& ie,
                                             const u32& tid) {
    constexpr u32 U = 8;
    for (u32 t0 = tid; t0 < ie.y; t0 += U * NT) {
        u32 pos[U];
#pragma unroll
        for (u32 k = 0; k < U; ++k) {
            const u32 t = t0 + k * NT;
            pos[k] = t < ie.y ? a.sortedPos[ie.x + t] : 0u;
        }
#pragma unroll
        for (u32 k = 0; k < U; ++k) {
            const u32 t = t0 + k * NT;
            if (t < ie.y) a.P[pos[k]] = res[t];
        }
    }
}

// Row-block SDDMM: one workgroup per work item {row block, kept-tile range, piece
// range}: the row block's A rows staged in LDS, then its MFMA tiles and column-run pieces, then
// (staged output) the item's results in CSR order. The steps are the functions above; the pair
// kernel's driver (rb_item) runs the same steps on two items.
// LITE: the form the C2-like launches take — no kept MFMA tiles, one store per entry (no staged
// output), default staging policy, phase-0 B after the barrier, no trace or ablations (launch_rb
// picks it only then): the same instructions on that path, without the code of the others
template <int DT, int RBY, int NT, bool DYN, bool LITE = false>
__global__ __launch_bounds__(NT, 4) void k_sddmm_rb(RbArgs a) {
    extern __shared__ __attribute__((aligned(16))) char AsB[];
    char* As = AsB;
    if (blockIdx.y) {  // batch b (item -> XCD placement unchanged: nItems is a multiple of 8)
        a.A += blockIdx.y * a.bA;
        a.B += blockIdx.y * a.bB;
        a.P += blockIdx.y * a.bP;
    }
    using Geo = RowGeom<RBY>;
    using SG = StageGeom<RBY, NT>;
    constexpr u32 G = Geo::G, NC = Geo::NC;  // lanes per entry, chunks per lane
    constexpr u32 NW = NT / 64;               // waves per workgroup
    constexpr u32 TC = DenseTileLds<DT, RBY>::CH;
    const u32 idx = blockIdx.x;
    const unsigned long long t0 = LITE ? 0ull : rtime(a.trace);
    uint4 it;
    u32 pend;
    if (rb_load_item(a, idx, it, pend)) return;  // padding
    const u32 q0 = a.qbase + it.x * a.RB;
    const u32 tid = threadIdx.x, w = tid >> 6, sub = tid % G, j = (tid & 63) / G;
    // every wave takes (at most) one dense tile and its row-groups one residual piece each per
    // phase; the first tile and the phase-0 pieces (B operand, metadata) are issued before the
    // staging loads so all of it is in flight together
    const u32 ntile = !LITE && (a.mode & 1) ? it.z - it.y : 0u;
    const u32 np = LITE || (a.mode & 2) ? pend - it.w : 0u;  // (lite: the whole launch, mode 3)
    const u32 gr = tid / G;
    u32 rot[NC];  // residual: byte offset of the G-chunk group the lane visits at step f
#pragma unroll
    for (u32 f = 0; f < NC; ++f) rot[f] = 16u * G * ((f + j % Geo::RR) % NC);
    // the staging by LDS-DMA: see rb_stage_issue
    const u32 lane = tid & 63;
    const u32 ws = __builtin_amdgcn_readfirstlane(w);  // wave index in an SGPR
    // the staging row indices are loaded first: they depend only on the item, so their round
    // trip overlaps the piece descriptor's, and the LDS-DMAs need not wait for the B columns
    u32 rowv = 0;
    u32 src[SG::NSRC];
    if constexpr (SG::ROWV)
        rowv = rb_stage_rows<RBY, NT>(a, q0, ws, lane);
    else {
        // 128-byte rows: 8 rows per block, too many indices for one per lane; each lane loads
        // the row of its own chunk for every block
#pragma unroll
        for (u32 i = 0; i < SG::MAXB; ++i) {
            const u32 lr = 64 * (ws + i * SG::NW) / SG::NCH + lane / SG::NCH, q = q0 + lr;
            src[i] = lr < a.RB && q < a.R ? a.rows[q] : a.row0;
        }
        // all row indices in registers before the first LDS-DMA: the compiler does not count
        // the (inline asm) DMAs, so a wait for a later index placed between them would also
        // wait for the DMAs issued before it (mycielskian14 K = 32: 16.3 -> 17.7 us)
#pragma unroll
        for (u32 i = 0; i < SG::MAXB; ++i) asm volatile("" : "+v"(src[i]));
    }
    // the loads the LDS-DMA issue waits for go first: row indices, the phase-0 piece descriptor
    // and the first tile's metadata (one round trip together); the B columns and entry metadata
    // they address are issued after the LDS-DMAs, so the staging never waits for a B gather
    f32x4 tb[TC], pre[NC];
    DenseTileLds<DT, RBY> dt;
    // tiles go to the last waves, which hold the shortest pieces (pieces are sorted longest first)
    const u32 tw = NW - 1 - w;
    Piece<RBY> pc;
    pc.len = 0;
    if constexpr (!LITE)
        if (tw < ntile) dt.meta(a, a.tileIds[it.y + tw], q0);
    if (gr < np) load_piece_desc<RBY>(a, it.w + gr, pc);
    // staged output by runs: this lane's run descriptor (run w + NW * lane of the item), loaded
    // in the item's last piece phase, where the next-phase prefetch registers are free, so the
    // store pass waits for nothing but the LDS slots
    uint2 myrun = make_uint2(0u, 0u), irun = make_uint2(0u, 0u);
    auto load_runs = [&]() {
        if (!LITE && a.runs && a.outLds) {
            irun = a.itemRuns[idx];
            irun.x = __builtin_amdgcn_readfirstlane(irun.x);
            irun.y = __builtin_amdgcn_readfirstlane(irun.y);
            const u32 jr = w + NW * lane;
            if (jr < irun.y) myrun = a.runs[irun.x + jr];
        }
    };
    // AUX: the LDS-DMA cache policy (0 default; 2 = nt, stream the A rows past the XCD's L2 so the
    // B columns of the item's column range stay resident: large staged-output layouts, where an
    // item's row block is not staged again on that XCD until the next range). The issue loop is
    // fully unrolled here (the pair rolls it by two)
    auto stage = [&](auto aux_tag) {
        constexpr int AUX = decltype(aux_tag)::value;
        if constexpr (SG::ROWV)
            rb_stage_issue<DT, RBY, NT, AUX, SG::MAXB>(a, As, rowv, ws, lane);
        else
            rb_stage_issue128<DT, RBY, NT, AUX>(a, As, src, ws, lane);
    };
    if (!LITE && a.stageNt)
        stage(std::integral_constant<int, 2>{});
    else
        stage(std::integral_constant<int, 0>{});
    // the phase-0 B columns and entry metadata: issued right behind the LDS-DMAs (so the
    // barrier's wait covers them too), or with lateB after the barrier (the barrier then waits
    // for the staging alone and the waves pay one load round trip before their first piece)
    if (!LITE && !a.lateB) {
        if (gr < np) load_piece_body<RBY>(a, sub, rot, pre, pc);
        if (tw < ntile) dt.loadB(a, 0, tb);
    }
    if constexpr (DYN)  // (the image-only staging never writes the last word)
        if (tid == 0) *rb_batch_ctr<NT>(As) = 0u;
    // every LDS-DMA of the workgroup has landed before any wave reads the image or writes the
    // staged-output slots (the blocks past the image land in the tail those slots use); explicit,
    // not left to the compiler's wait insertion at the barrier
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (LITE || a.lateB) {
        if (gr < np) load_piece_body<RBY>(a, sub, rot, pre, pc);
        if constexpr (!LITE)
            if (tw < ntile) dt.loadB(a, 0, tb);
    }
    const unsigned long long tm = LITE ? 0ull : rtime(a.trace);
    if (!LITE && (a.diag & 8)) {  // staging only
        trace_wave(a.trace, idx * NW + w, t0, tm);
        return;
    }
    if constexpr (!LITE)
        if (tw < ntile) dt.run(a, As, tb);
    const unsigned long long td = LITE ? 0ull : rtime(a.trace);
    if constexpr (DYN)
        rb_batches<DT, RBY, NT>(a, As, it.w, np, gr, sub, rot, pc, pre, load_runs);
    else {
        constexpr u32 NG = NT / G;  // residual row-groups
        Piece<RBY> pn;
        f32x4 nb[NC];
        auto fetch = [&](const u32 ph) {
            const u32 pi = ph * NG + ((ph & 1) ? NG - 1 - gr : gr);
            pn.len = 0;
            if (pi < np) load_piece<RBY>(a, it.w + pi, sub, rot, nb, pn);
        };
        if (NG < np)
            fetch(1);
        else
            load_runs();
        if (pc.len) residual_piece<DT, RBY>(a, As, pc, sub, rot, pre);
        for (u32 ph = 1; ph * NG < np; ++ph) {
            pc = pn;
#pragma unroll
            for (u32 f = 0; f < NC; ++f) pre[f] = nb[f];
            if ((ph + 1) * NG < np)
                fetch(ph + 1);
            else
                load_runs();
            if (pc.len) residual_piece<DT, RBY>(a, As, pc, sub, rot, pre);
        }
    }
    if constexpr (LITE) return;
    for (u32 t = it.y + tw + NW; t < it.z; t += NW) {  // tiles beyond one per wave
        dt.load(a, a.tileIds[t], q0, tb);
        dt.run(a, As, tb);
    }
    if (a.outLds) {  // the item's results in CSR order: runs of consecutive positions
        __syncthreads();
        const uint2 ie = a.itemEnt[idx];
        const float* res = reinterpret_cast<const float*>(As + a.outLds);
        if (!(a.diag & 128)) {  // (BSMR_DIAG & 128, ablation only: no P stores)
            auto pass = [&]() { store_sorted<NT>(a, res, ie, tid); };
            if (a.runs) {
                // wave w writes runs w, w + NW, ...: one contiguous store of up to 64 results
                // per run (a row's results in this item, when rows are column-sorted), four
                // runs per step with their LDS reads in flight together
                const u32 nr = irun.y > w ? (irun.y - w + NW - 1) / NW : 0u;
                for (u32 i = 0; i < nr; i += 4) {
                    u32 pos[4], s0[4], len[4];
                    float v[4];
#pragma unroll
                    for (u32 u = 0; u < 4; ++u) {
                        const u32 q = min(i + u, 63u);
                        pos[u] = static_cast<u32>(__builtin_amdgcn_readlane(static_cast<int>(myrun.x), q));
                        const u32 sl = static_cast<u32>(__builtin_amdgcn_readlane(static_cast<int>(myrun.y), q));
                        s0[u] = sl & 0xFFFFu;
                        len[u] = i + u < nr ? sl >> 16 : 0u;
                        v[u] = lane < len[u] ? res[s0[u] + lane] : 0.0f;
                    }
#pragma unroll
                    for (u32 u = 0; u < 4; ++u)  // (runs are at most 64 long)
                        if (lane < len[u]) a.P[pos[u] + lane] = v[u];
                }
            } else {
                pass();
            }
        }
    }
    trace_wave(a.trace, idx * NW + w, t0, tm, td);
}

// One item of the pair kernel (staged output by runs, no kept MFMA tiles, late B loads, default
// staging policy, no trace or ablations: launch_rb picks the kernel only then, and its two items
// fit the SGPR budget without those paths): the steps of k_sddmm_rb, see there. prestaged: the
// previous item of the workgroup's pair already issued this item's staging. next: the item that
// runs next on this workgroup; its staging is issued in this item's store pass, right after the
// result slots have been read into registers, so the next image lands while this item's stores
// drain. Returns whether next's staging was issued (false: no next, next is padding, or this
// item is).
template <int DT, int RBY, int NT, bool DYN>
__device__ __forceinline__ bool rb_item(const RbArgs& a, char* As, const u32 idx, const bool prestaged,
                                        const u32 next) {
    using Geo = RowGeom<RBY>;
    using SG = StageGeom<RBY, NT>;
    constexpr u32 G = Geo::G, NC = Geo::NC;  // lanes per entry, chunks per lane
    constexpr u32 NW = NT / 64;               // waves per workgroup
    uint4 it;
    u32 pend;
    if (rb_load_item(a, idx, it, pend)) return false;  // padding
    // the next item of the pair: its row block (its staging rows are loaded behind the pieces)
    bool has_next = false, same_rb = false;
    u32 q0n = 0;
    if (next != NO_ITEM) {
        uint4 nt = a.items[next];
        nt.x = __builtin_amdgcn_readfirstlane(nt.x);
        nt.y = __builtin_amdgcn_readfirstlane(nt.y);
        nt.z = __builtin_amdgcn_readfirstlane(nt.z);
        nt.w = __builtin_amdgcn_readfirstlane(nt.w);
        const u32 nend = __builtin_amdgcn_readfirstlane(a.itemEnd[next]);
        has_next = !(nt.y == nt.z && nt.w == nend);
        q0n = a.qbase + nt.x * a.RB;
        // the same row block (consecutive chunks of one segment): its image is already in LDS
        // (the pieces only read it; the slots live past it), so nothing is staged again
        same_rb = nt.x == it.x;
    }
    const u32 q0 = a.qbase + it.x * a.RB;
    u32 tid = threadIdx.x;
    // two items per workgroup: the thread-derived values are recomputed per item rather than
    // hoisted out of the caller's sequence, where they would hold VGPRs across it
    asm volatile("" : "+v"(tid));
    const u32 w = tid >> 6, sub = tid % G, j = (tid & 63) / G;
    const u32 np = (a.mode & 2) ? pend - it.w : 0u;
    const u32 gr = tid / G;
    u32 rot[NC];
#pragma unroll
    for (u32 f = 0; f < NC; ++f) rot[f] = 16u * G * ((f + j % Geo::RR) % NC);
    const u32 lane = tid & 63;
    const u32 ws = __builtin_amdgcn_readfirstlane(w);  // wave index in an SGPR
    u32 rowv = 0;  // (set before every staging: rb_stage_rows, or the next item's rows)
    u32 src[SG::NSRC];
    if (!prestaged) {
        rowv = rb_stage_rows<RBY, NT>(a, q0, ws, lane);
    }
    f32x4 pre[NC];
    Piece<RBY> pc;
    pc.len = 0;
    if (gr < np) load_piece_desc<RBY>(a, it.w + gr, pc);
    // this lane's run descriptor and, with a next item, its staging row indices: loaded behind
    // the pieces, not in their last phase: live across the phase loop, they cost the loop VGPRs;
    // a wave that ends early has them back before the store-pass barrier
    uint2 myrun = make_uint2(0u, 0u), irun = make_uint2(0u, 0u);
    u32 rown = a.row0;
    auto load_runs = [&]() {
        if (a.runs && a.outLds) {
            irun = a.itemRuns[idx];
            irun.x = __builtin_amdgcn_readfirstlane(irun.x);
            irun.y = __builtin_amdgcn_readfirstlane(irun.y);
            const u32 jr = w + NW * lane;
            if (jr < irun.y) myrun = a.runs[irun.x + jr];
        }
        if (has_next && !same_rb) rown = rb_stage_rows<RBY, NT>(a, q0n, ws, lane);
    };
    // the issue loop rolled by two: fully unrolled, its v_readlane results were all hoisted into
    // SGPRs, which the two items cannot spare
    auto stage = [&]() {
        if constexpr (SG::ROWV)
            rb_stage_issue<DT, RBY, NT, 0, 2>(a, As, rowv, ws, lane);
        else
            rb_stage_issue128<DT, RBY, NT, 0>(a, As, src, ws, lane);
    };
    if (!prestaged) stage();
    // the batch counter (no LDS-DMA writes the last word; every grab of the pair's previous item
    // ended before its store-pass barrier)
    if constexpr (DYN)
        if (tid == 0) *rb_batch_ctr<NT>(As) = 0u;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (gr < np) load_piece_body<RBY>(a, sub, rot, pre, pc);
    if constexpr (DYN)
        rb_batches<DT, RBY, NT>(a, As, it.w, np, gr, sub, rot, pc, pre, [] {});
    else {
        constexpr u32 NG = NT / G;  // residual row-groups
        Piece<RBY> pn;
        f32x4 nb[NC];
        auto fetch = [&](const u32 ph) {
            const u32 pi = ph * NG + ((ph & 1) ? NG - 1 - gr : gr);
            pn.len = 0;
            if (pi < np) load_piece<RBY>(a, it.w + pi, sub, rot, nb, pn);
        };
        if (NG < np) fetch(1);
        if (pc.len) residual_piece<DT, RBY>(a, As, pc, sub, rot, pre);
        for (u32 ph = 1; ph * NG < np; ++ph) {
            pc = pn;
#pragma unroll
            for (u32 f = 0; f < NC; ++f) pre[f] = nb[f];
            if ((ph + 1) * NG < np) fetch(ph + 1);
            if (pc.len) residual_piece<DT, RBY>(a, As, pc, sub, rot, pre);
        }
    }
    load_runs();
    bool staged_next = false;
    if (a.outLds) {  // the item's results in CSR order: runs of consecutive positions
        __syncthreads();
        const float* res = reinterpret_cast<const float*>(As + a.outLds);
        const u32 nr = irun.y > w ? (irun.y - w + NW - 1) / NW : 0u;  // runs w, w + NW, ...
        if constexpr (SG::ROWV) {
            // this wave's run values into registers, a barrier (no wave reads a slot any more;
            // the next image may reach into the slots), the next item's LDS-DMAs, then this
            // item's stores, all in flight together. (An item that holds more runs per wave than
            // PAIR_RUNS_PER_WAVE stores them the plain way, below.)
            if (has_next && __builtin_amdgcn_readfirstlane(irun.y) <= NW * PAIR_RUNS_PER_WAVE) {
                float v[PAIR_RUNS_PER_WAVE];
#pragma unroll
                for (u32 u = 0; u < PAIR_RUNS_PER_WAVE; ++u) {
                    const u32 sl = static_cast<u32>(__builtin_amdgcn_readlane(static_cast<int>(myrun.y), u));
                    const u32 len = u < nr ? sl >> 16 : 0u;
                    v[u] = lane < len ? res[(sl & 0xFFFFu) + lane] : 0.0f;
                }
                __syncthreads();
                rowv = rown;
                if (!same_rb) stage();
#pragma unroll
                for (u32 u = 0; u < PAIR_RUNS_PER_WAVE; ++u) {
                    const u32 pos = static_cast<u32>(__builtin_amdgcn_readlane(static_cast<int>(myrun.x), u));
                    const u32 sl = static_cast<u32>(__builtin_amdgcn_readlane(static_cast<int>(myrun.y), u));
                    const u32 len = u < nr ? sl >> 16 : 0u;
                    if (lane < len) a.P[pos + lane] = v[u];
                }
                return true;
            }
        }
        // the plain way: as in k_sddmm_rb
        for (u32 i = 0; i < nr; i += 4) {
            u32 pos[4], s0[4], len[4];
            float v[4];
#pragma unroll
            for (u32 u = 0; u < 4; ++u) {
                const u32 q = min(i + u, 63u);
                pos[u] = static_cast<u32>(__builtin_amdgcn_readlane(static_cast<int>(myrun.x), q));
                const u32 sl = static_cast<u32>(__builtin_amdgcn_readlane(static_cast<int>(myrun.y), q));
                s0[u] = sl & 0xFFFFu;
                len[u] = i + u < nr ? sl >> 16 : 0u;
                v[u] = lane < len[u] ? res[s0[u] + lane] : 0.0f;
            }
#pragma unroll
            for (u32 u = 0; u < 4; ++u)  // (runs are at most 64 long)
                if (lane < len[u]) a.P[pos[u] + lane] = v[u];
        }
        // the first item stored the plain way: the next image is staged now (every slot read
        // has completed at the barrier)
        if constexpr (SG::ROWV) {
            if (has_next) {
                __syncthreads();
                rowv = rown;
                if (!same_rb) stage();
                staged_next = true;
            }
        }
    }
    return staged_next;
}


// Pairs (staged output by runs): a workgroup runs list positions 2j and 2j + 1 of its XCD
// (items are laid out [position * 8 + x]; workgroup g runs on XCD g % 8), the second item's
// staging issued in the first one's store pass (rb_item)
template <int DT, int RBY, int NT, bool DYN>
__global__ __launch_bounds__(NT, 4) void k_sddmm_rb_pair(RbArgs a) {
    extern __shared__ __attribute__((aligned(16))) char AsB[];
    char* As = AsB;
    if (blockIdx.y) {  // batch b
        a.A += blockIdx.y * a.bA;
        a.B += blockIdx.y * a.bB;
        a.P += blockIdx.y * a.bP;
    }
    const u32 x = blockIdx.x % XCD_BUCKETS, i0 = (blockIdx.x / XCD_BUCKETS) * 2 * XCD_BUCKETS + x;
    if (rb_item<DT, RBY, NT, DYN>(a, As, i0, false, i0 + XCD_BUCKETS))
        rb_item<DT, RBY, NT, DYN>(a, As, i0 + XCD_BUCKETS, true, NO_ITEM);
}

template <int DT, int RBY>
void (*pick_rb(const u32 NT, const bool pairs, const bool dyn, const bool lite))(RbArgs) {
    // (dynamic batches: rows of <= 512 B, RowBlockLayout::dynBatches)
    if constexpr (RBY >= 256) {  // (launch_rb enables pairs from 512-byte rows)
        if (pairs) {
            if constexpr (RBY <= 512)
                if (dyn) return NT == 1024 ? k_sddmm_rb_pair<DT, RBY, 1024, true> : k_sddmm_rb_pair<DT, RBY, 512, true>;
            return NT == 1024 ? k_sddmm_rb_pair<DT, RBY, 1024, false> : k_sddmm_rb_pair<DT, RBY, 512, false>;
        }
    }
    if constexpr (RBY <= 512)
        if (dyn) {
            if (lite) return NT == 1024 ? k_sddmm_rb<DT, RBY, 1024, true, true> : k_sddmm_rb<DT, RBY, 512, true, true>;
            return NT == 1024 ? k_sddmm_rb<DT, RBY, 1024, true> : k_sddmm_rb<DT, RBY, 512, true>;
        }
    if (lite) return NT == 1024 ? k_sddmm_rb<DT, RBY, 1024, false, true> : k_sddmm_rb<DT, RBY, 512, false, true>;
    return NT == 1024 ? k_sddmm_rb<DT, RBY, 1024, false> : k_sddmm_rb<DT, RBY, 512, false>;
}

}  // namespace
}  // namespace bsmr
