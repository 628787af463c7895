// capi.cpp — plan lifecycle, parity dumps, reorder statistics and sharding of the C ABI.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "plan.hpp"

using namespace bsmr;

namespace {

// device, stream and the launch / tuning options shared by bsmr_plan_create and
// bsmr_plan_import_rows
int init_plan(Plan& p, const bsmr_plan_options& o) {
    p.device = o.device;
    if (hipSetDevice(o.device) != hipSuccess) {
        set_error("bsmr_plan: hipSetDevice failed");
        return BSMR_ERR_HIP;
    }
    if (hipStreamCreateWithFlags(&p.stream, hipStreamNonBlocking) != hipSuccess) {
        set_error("bsmr_plan: hipStreamCreate failed");
        return BSMR_ERR_HIP;
    }
    p.alpha = o.alpha;
    p.delta = o.delta;
    p.exact_all = o.exact_similarity;
    return report(apply_options(p.k, o));
}

// The CSR contract of bsmr_plan_create / bsmr_plan_import_rows (include/bsmr.h), checked on the
// host in O(M + nnz) before any device call: k_encode indexes an LDS histogram of nbpr words by
// col / bs and walks rowptr[r] .. rowptr[r + 1], so a column >= N or a decreasing rowptr would
// write out of bounds on the device. Returns false with the first offender in bsmr_last_error.
bool valid_csr(const char* who, const uint32_t* rowptr, const uint32_t* colidx, uint32_t M,
               uint32_t N, uint32_t nnz) {
    if (!(rowptr && colidx && M != 0 && N != 0 && rowptr[M] == nnz && nnz >= 2)) {
        set_error(std::string(who) + ": invalid CSR (need rowptr[M] == nnz >= 2)");
        return false;
    }
    if (rowptr[0] != 0) {
        set_error(std::string(who) + ": invalid CSR (rowptr[0] = " + std::to_string(rowptr[0]) +
                  ", need 0)");
        return false;
    }
    for (uint32_t r = 0; r < M; ++r)
        if (rowptr[r] > rowptr[r + 1]) {
            set_error(std::string(who) + ": invalid CSR (rowptr decreases at row " +
                      std::to_string(r) + ": " + std::to_string(rowptr[r]) + " > " +
                      std::to_string(rowptr[r + 1]) + ")");
            return false;
        }
    for (uint32_t k = 0; k < nnz; ++k)
        if (colidx[k] >= N) {
            set_error(std::string(who) + ": invalid CSR (colidx[" + std::to_string(k) + "] = " +
                      std::to_string(colidx[k]) + " >= N = " + std::to_string(N) + ")");
            return false;
        }
    return true;
}

}  // namespace

extern "C" int bsmr_plan_create(const uint32_t* rowptr, const uint32_t* colidx, uint32_t M,
                                uint32_t N, uint32_t nnz, const bsmr_plan_options* opt,
                                bsmr_plan** out) {
    *out = nullptr;
    if (!valid_csr("bsmr_plan_create", rowptr, colidx, M, N, nnz)) return BSMR_ERR_INVALID;
    bsmr_plan_options o;
    if (opt)
        o = *opt;
    else
        bsmr_plan_options_default(&o);
    auto* h = new bsmr_plan;
    Plan& p = h->p;
    auto fail = [&](int st) {
        delete h;
        return st;
    };
    p.M = M;
    p.N = N;
    p.nnz = nnz;
    int st = init_plan(p, o);
    if (st != BSMR_OK) return fail(st);
    u64 free_mem = o.free_mem_bytes;
    if (free_mem == 0) {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) {
            set_error("bsmr_plan_create: hipMemGetInfo failed");
            return fail(BSMR_ERR_HIP);
        }
        free_mem = fr;
    }
    p.bs = block_size_for(M, N, free_mem);
    if (p.bs > 65535) {
        set_error("bsmr_plan_create: column block size exceeds 16-bit encoding");
        return fail(BSMR_ERR_UNSUPPORTED);
    }
    p.nbpr = static_cast<u32>(std::ceil(static_cast<float>(N) / static_cast<float>(p.bs)));  // rowReordering.cu:1035
    p.B = cluster_block_dim(p.nbpr);
    p.keptMask = kept_warp_mask(p.B);
    st = p.build_rows(rowptr, colidx);
    if (st != BSMR_OK) return fail(st);
    st = p.build_columns();
    if (st != BSMR_OK) return fail(st);
    *out = h;
    return BSMR_OK;
}

extern "C" int bsmr_plan_export_rows(const bsmr_plan* plan, bsmr_row_stage* hdr, uint32_t* rows) {
    if (!plan || !hdr) {
        set_error("bsmr_plan_export_rows: bad arguments");
        return BSMR_ERR_INVALID;
    }
    const Plan& p = plan->p;
    std::memset(hdr, 0, sizeof(*hdr));
    hdr->M = p.M;
    hdr->N = p.N;
    hdr->nnz = p.nnz;
    hdr->block_size = p.bs;
    hdr->num_blocks_per_row = p.nbpr;
    hdr->cluster_block_dim = p.B;
    hdr->num_zero_rows = p.z;
    hdr->num_reordered_rows = p.R;
    hdr->num_clusters = p.numClusters;
    hdr->alpha = p.alpha;
    hdr->row_reorder_ms = p.row_ms;
    hdr->exact_similarity_evals = p.exact_evals;
    hdr->total_similarity_evals = p.total_evals;
    if (rows && p.R) {
        BSMR_HIP(hipSetDevice(p.device));
        BSMR_HIP(hipMemcpyAsync(rows, p.rows.data(), static_cast<size_t>(p.R) * sizeof(u32),
                                hipMemcpyDefault, p.stream));
        BSMR_HIP(hipStreamSynchronize(p.stream));
    }
    return BSMR_OK;
}

extern "C" int bsmr_plan_import_rows(const uint32_t* rowptr, const uint32_t* colidx,
                                     const bsmr_row_stage* hdr, const uint32_t* rows,
                                     const bsmr_plan_options* opt, bsmr_plan** out) {
    *out = nullptr;
    if (!hdr) {
        set_error("bsmr_plan_import_rows: invalid CSR or row-stage header");
        return BSMR_ERR_INVALID;
    }
    if (!valid_csr("bsmr_plan_import_rows", rowptr, colidx, hdr->M, hdr->N, hdr->nnz))
        return BSMR_ERR_INVALID;
    if (hdr->num_reordered_rows > hdr->M || hdr->num_zero_rows > hdr->M ||
        hdr->num_reordered_rows + hdr->num_zero_rows != hdr->M ||
        (hdr->num_reordered_rows && !rows)) {
        set_error("bsmr_plan_import_rows: invalid CSR or row-stage header");
        return BSMR_ERR_INVALID;
    }
    bsmr_plan_options o;
    if (opt)
        o = *opt;
    else
        bsmr_plan_options_default(&o);
    o.alpha = hdr->alpha;  // the row stage was built for this alpha; delta comes from opt
    auto* h = new bsmr_plan;
    Plan& p = h->p;
    auto fail = [&](int st) {
        delete h;
        return st;
    };
    const u32 M = hdr->M, R = hdr->num_reordered_rows;
    p.M = M;
    p.N = hdr->N;
    p.nnz = hdr->nnz;
    int st = init_plan(p, o);
    if (st != BSMR_OK) return fail(st);
    // the column-stage geometry must be the one bsmr_plan_create derives from (M, N, bs)
    // (rowReordering.cu:1035, 911-920); bs itself depends on the exporter's free memory
    if (hdr->block_size < 16 || hdr->block_size > 65535 ||
        hdr->num_blocks_per_row !=
            static_cast<u32>(std::ceil(static_cast<float>(hdr->N) / static_cast<float>(hdr->block_size))) ||
        hdr->cluster_block_dim != cluster_block_dim(hdr->num_blocks_per_row)) {
        set_error("bsmr_plan_import_rows: block_size / num_blocks_per_row / cluster_block_dim "
                  "inconsistent with N");
        return fail(BSMR_ERR_INVALID);
    }
    // the rows must be the non-empty rows of S, each once (they index rowptr on the device):
    // num_zero_rows equal to S's empty-row count, R distinct non-empty rows, R + z == M
    u32 empty = 0;
    for (u32 r = 0; r < M; ++r) empty += rowptr[r] == rowptr[r + 1];
    if (empty != hdr->num_zero_rows) {
        set_error("bsmr_plan_import_rows: num_zero_rows differs from the empty rows of S");
        return fail(BSMR_ERR_INVALID);
    }
    std::vector<u32> hrows(R);
    if (R && hipMemcpy(hrows.data(), rows, static_cast<size_t>(R) * sizeof(u32), hipMemcpyDefault) !=
                 hipSuccess) {
        set_error("bsmr_plan_import_rows: cannot read rows");
        return fail(BSMR_ERR_HIP);
    }
    std::vector<uint8_t> seen(M, 0);
    for (u32 r : hrows) {
        if (r >= M || seen[r] || rowptr[r] == rowptr[r + 1]) {
            set_error("bsmr_plan_import_rows: rows are not the non-empty rows of S, each once");
            return fail(BSMR_ERR_INVALID);
        }
        seen[r] = 1;
    }
    p.bs = hdr->block_size;
    p.nbpr = hdr->num_blocks_per_row;
    p.B = hdr->cluster_block_dim;
    p.keptMask = kept_warp_mask(p.B);
    p.z = hdr->num_zero_rows;
    p.R = R;
    p.P = (R + 15) / 16;
    p.numClusters = hdr->num_clusters;
    p.row_ms = hdr->row_reorder_ms;
    p.exact_evals = hdr->exact_similarity_evals;
    p.total_evals = hdr->total_similarity_evals;
    st = p.rowptr.upload(rowptr, M + 1ull, p.stream);
    if (st == BSMR_OK) st = p.colidx.upload(colidx, p.nnz, p.stream);
    if (st == BSMR_OK) st = p.rows.upload(hrows.data(), R, p.stream);  // R >= 1: nnz >= 2
    if (st == BSMR_OK) st = p.build_columns();
    if (st != BSMR_OK) return fail(st);
    *out = h;
    return BSMR_OK;
}

extern "C" int bsmr_plan_recolumn(bsmr_plan* plan, float delta) {
    if (!plan) return BSMR_ERR_INVALID;
    plan->p.delta = delta;
    return plan->p.build_columns();
}

extern "C" void bsmr_plan_destroy(bsmr_plan* plan) { delete plan; }

extern "C" int bsmr_plan_get_stats(const bsmr_plan* plan, bsmr_plan_stats* s) {
    if (!plan || !s) return BSMR_ERR_INVALID;
    const Plan& p = plan->p;
    std::memset(s, 0, sizeof(*s));
    s->M = p.M;
    s->N = p.N;
    s->nnz = p.nnz;
    s->block_size = p.bs;
    s->num_blocks_per_row = p.nbpr;
    s->cluster_block_dim = p.B;
    s->num_clusters = p.numClusters;
    s->num_row_panels = p.P;
    s->num_reordered_rows = p.R;
    s->num_dense_tiles = p.numDenseTiles;
    s->max_dense_tiles_per_panel = p.maxTilesPerPanel;
    s->num_residual = p.nres;
    s->num_dense_thread_blocks = p.numDenseTB;
    s->num_sparse_thread_blocks = p.numSparseTB;
    s->exact_similarity_evals = p.exact_evals;
    s->total_similarity_evals = p.total_evals;
    s->row_reorder_ms = p.row_ms;
    s->cluster_filter_used = p.filter_used ? 1u : 0u;
    s->cluster_filter_ms = p.filter_ms;
    s->col_reorder_ms = p.col_ms;
    s->dense_items = p.nDenseItems;
    s->residual_items = p.nResItems;
    for (int i = 0; i < Plan::N_RB_SIZES; ++i) {  // per row size: the fp32 layout, else the half one
        const Plan::RowBlockLayout& L = p.rbl[i].rowBytes ? p.rb_whole(i) : p.rb_whole(i + Plan::N_RB_SIZES);
        s->rb_rows[i] = L.rowBytes ? L.RB : 0;
        s->rb_items[i] = L.rowBytes ? L.nItems : 0;
        s->rb_pieces[i] = L.rowBytes ? L.nPieces : 0;
        s->rb_entries[i] = L.rowBytes ? L.nEntries : 0;
        s->rb_tiles[i] = L.rowBytes ? L.nTilesKept : 0;
        s->rb_work_items[i] = L.rowBytes ? L.nWorkItems : 0;
        if (L.rowBytes && L.orig) s->rb_orig_rows |= 1u << i;
        if (L.rowBytes && L.cols) s->rb_col_blocks |= 1u << i;
        if (L.rowBytes && rb_form(rb_layout_facts(L), p.k, 3).pairs) s->rb_pairs |= 1u << i;
        if (L.rowBytes && L.dynBatches) s->rb_batches |= 1u << i;
    }
    s->dense_sampled_tiles = p.dense.built ? p.dense.nonempty : 0;
    s->ptile_items = p.ptile.built ? p.ptile.nItems : 0;
    return BSMR_OK;
}

extern "C" int bsmr_plan_get_array(const bsmr_plan* plan, int which, uint32_t* host_out,
                                   uint64_t* len) {
    if (!plan) return BSMR_ERR_INVALID;
    const Plan& p = plan->p;
    const DevBuf<u32>* b = nullptr;
    size_t n = 0;
    switch (which) {
        case BSMR_ARR_REORDERED_ROWS: b = &p.rows; n = p.R; break;
        case BSMR_ARR_DENSE_COLS: b = &p.denseCols; n = p.denseCols.n; break;
        case BSMR_ARR_DENSE_COL_OFFSETS: b = &p.denseColOffsets; n = p.P + 1; break;
        case BSMR_ARR_SPARSE_COLS: b = &p.sparseCols; n = p.sparseCols.n; break;
        case BSMR_ARR_SPARSE_COL_OFFSETS: b = &p.sparseColOffsets; n = p.P + 1; break;
        case BSMR_ARR_SPARSE_VALUE_OFFSETS: b = &p.sparseValueOffsets; n = p.P + 1; break;
        case BSMR_ARR_BLOCK_OFFSETS: b = &p.blockOffsets; n = p.P + 1; break;
        case BSMR_ARR_BLOCK_VALUES: b = &p.blockValues; n = p.blockValues.n; break;
        case BSMR_ARR_SPARSE_VALUES: b = &p.sparseValues; n = p.nres; break;
        case BSMR_ARR_SPARSE_RELATIVE_ROWS: b = &p.sparseRel; n = p.nres; break;
        case BSMR_ARR_SPARSE_COL_INDICES: b = &p.sparseColIdx; n = p.nres; break;
        // (not kept by plans imported from a row stage: length 0)
        case BSMR_ARR_DISPERSION: b = &p.disp; n = p.disp.n ? p.M : 0; break;
        case BSMR_ARR_ASCENDING: b = &p.asc; n = p.asc.n ? p.M : 0; break;
        default:
            set_error("bsmr_plan_get_array: unknown array");
            return BSMR_ERR_INVALID;
    }
    if (len) *len = n;
    if (host_out && n) {
        BSMR_HIP(hipSetDevice(p.device));
        BSMR_HIP(hipMemcpy(host_out, b->data(), n * sizeof(u32), hipMemcpyDeviceToHost));
    }
    return BSMR_OK;
}

// evaluationReordering + calculateNumDenseBlocksAndAverageDensityInOriginalMatrix
// (BSMR.cpp:826-930, 955-994), evaluated on the host from the plan arrays (log statistics only;
// not on the timed path). Float accumulation order follows the reference loops.
extern "C" int bsmr_plan_evaluate(const bsmr_plan* plan, bsmr_eval_stats* out) {
    if (!plan || !out) return BSMR_ERR_INVALID;
    const Plan& p = plan->p;
    BSMR_HIP(hipSetDevice(p.device));
    std::vector<u32> rowptr, col, rows, dco, dcols, sco, scols;
    BSMR_CHECK(p.rowptr.download(rowptr, p.stream));
    BSMR_CHECK(p.colidx.download(col, p.stream));
    BSMR_CHECK(p.rows.download(rows, p.stream));
    BSMR_CHECK(p.denseColOffsets.download(dco, p.stream));
    BSMR_CHECK(p.denseCols.download(dcols, p.stream));
    BSMR_CHECK(p.sparseColOffsets.download(sco, p.stream));
    BSMR_CHECK(p.sparseCols.download(scols, p.stream));
    rows.resize(p.R);
    const u32 N = p.N;
    int numDense = 0, numSparseData = 0;
    float total = 0.f;
    std::vector<u32> blockOf(N + 1, NULLV);
    std::vector<char> isSparse(N + 1, 0);
    for (u32 q = 0; q < p.P; ++q) {
        const u32 d0 = dco[q], d1 = dco[q + 1], s0 = sco[q], s1 = sco[q + 1];
        const u32 nDB = (d1 - d0 + 15) / 16;
        for (u32 j = d0; j < d1; ++j) blockOf[dcols[j]] = (j - d0) / 16;
        for (u32 j = s0; j < s1; ++j) isSparse[scols[j]] = 1;
        std::vector<u32> cnt(nDB, 0);
        const u32 r1 = std::min(q * 16 + 16, p.R);
        for (u32 x = q * 16; x < r1; ++x)
            for (u32 k = rowptr[rows[x]]; k < rowptr[rows[x] + 1]; ++k) {
                if (blockOf[col[k]] != NULLV) ++cnt[blockOf[col[k]]];
                if (isSparse[col[k]]) ++numSparseData;
            }
        for (u32 b = 0; b < nDB; ++b)
            if (cnt[b] > 0) {
                const float density = static_cast<float>(cnt[b]) / 256.0f;
                total += density;
                if (density >= p.delta) ++numDense;
            }
        for (u32 j = d0; j < d1; ++j) blockOf[dcols[j]] = NULLV;
        for (u32 j = s0; j < s1; ++j) isSparse[scols[j]] = 0;
    }
    out->num_dense_block = numDense;
    const float avg = total / static_cast<float>(numDense);
    out->average_density = avg > 0 ? avg : 0.0f;
    out->num_sparse_data = numSparseData;
    out->num_dense_data = static_cast<int32_t>(p.nnz) - numSparseData;
    // original-order tiles
    const u32 OP = (p.M + 15) / 16;
    u32 onum = 0;
    float ototal = 0.f;
    std::vector<u32> cb;
    for (u32 q = 0; q < OP; ++q) {
        cb.clear();
        const u32 r0 = q * 16, r1 = std::min(r0 + 16, p.M);
        for (u32 r = r0; r < r1; ++r)
            for (u32 k = rowptr[r]; k < rowptr[r + 1]; ++k) cb.push_back(col[k] / 16);
        std::sort(cb.begin(), cb.end());
        for (size_t k = 0; k < cb.size();) {
            size_t j = k;
            while (j < cb.size() && cb[j] == cb[k]) ++j;
            const u32 c0 = cb[k] * 16, c1 = std::min(c0 + 16, N);
            const float bsz = static_cast<float>((r1 - r0) * (c1 - c0));
            const float density = static_cast<float>(j - k) / bsz;
            if (density >= p.delta) {
                ototal += density;
                ++onum;
            }
            k = j;
        }
    }
    out->original_num_dense_block = static_cast<int32_t>(onum);
    out->original_average_density = onum > 0 ? ototal / static_cast<float>(onum) : 0.0f;
    return BSMR_OK;
}

// Contiguous panel ranges balanced by a cost model: a dense tile costs 256*K MACs on the matrix
// core, priced at 1/4 of a residual MAC (fp32 MFMA vs. gathered scalar FMA); a residual entry
// costs K; every panel costs 1 (its A rows). cuts[0] = 0, cuts[world] = P, non-decreasing.
extern "C" int bsmr_shard_cuts(const uint32_t* blockOffsets, const uint32_t* sparseValueOffsets,
                               uint32_t P, uint32_t K, int world, uint32_t* cuts) {
    if (!blockOffsets || !sparseValueOffsets || !cuts || world <= 0) {
        set_error("bsmr_shard_cuts: bad arguments");
        return BSMR_ERR_INVALID;
    }
    std::vector<double> cum(P + 1ull, 0.0);
    for (u32 q = 0; q < P; ++q) {
        const double tiles = blockOffsets[q + 1] - blockOffsets[q];
        const double res = sparseValueOffsets[q + 1] - sparseValueOffsets[q];
        cum[q + 1] = cum[q] + tiles * 64.0 * K + res * K + 1.0;
    }
    cuts[0] = 0;
    for (int r = 1; r < world; ++r) {
        const double target = cum[P] * r / world;
        u32 c = static_cast<u32>(std::lower_bound(cum.begin(), cum.end(), target) - cum.begin());
        c = std::min(std::max(c, cuts[r - 1]), P);
        cuts[r] = c;
    }
    cuts[world] = P;
    return BSMR_OK;
}

extern "C" int bsmr_plan_shard(const bsmr_plan* plan, uint32_t K, int rank, int world,
                               uint32_t* p0, uint32_t* p1) {
    return bsmr_plan_shard_dtype(plan, K, BSMR_F32, rank, world, p0, p1);
}

namespace {
// cut [0, nRB) row blocks of cumulative cost cum (size nRB + 1) into `world` contiguous ranges,
// each cut at the row-block boundary closest to its target; cuts are panel indices
void cut_row_blocks(const std::vector<double>& cum, u32 nRB, u32 ppr, u32 P, int world, u32* cuts) {
    cuts[0] = 0;
    for (int r = 1; r < world; ++r) {
        const double target = cum[nRB] * r / world;
        u32 b = static_cast<u32>(std::lower_bound(cum.begin(), cum.end(), target) - cum.begin());
        if (b > 0 && target - cum[b - 1] < cum[std::min(b, nRB)] - target) --b;
        cuts[r] = std::max(cuts[r - 1], std::min(b * ppr, P));
    }
    cuts[world] = P;
}
}  // namespace

extern "C" int bsmr_cost_cuts(const double* block_cost, uint32_t nblocks, uint32_t panels_per_block,
                              uint32_t P, int world, const uint32_t* prev_cuts,
                              const float* shard_ms, uint32_t* cuts) {
    if ((!block_cost && nblocks) || world <= 0 || !cuts || panels_per_block == 0 ||
        (!prev_cuts) != (!shard_ms)) {
        set_error("bsmr_cost_cuts: bad arguments");
        return BSMR_ERR_INVALID;
    }
    const u32 nRB = nblocks, ppr = panels_per_block;
    std::vector<double> scale(nRB, 1.0);
    double norm = 1.0;
    if (prev_cuts) {
        if (prev_cuts[0] != 0 || prev_cuts[world] != P) {
            set_error("bsmr_plan_shard_rebalance: previous cuts must span [0, P]");
            return BSMR_ERR_INVALID;
        }
        // each block's model cost scaled by its shard's measured / predicted time
        std::vector<char> measured(nRB, 0);
        for (int r = 0; r < world; ++r) {
            if (prev_cuts[r + 1] < prev_cuts[r] || (prev_cuts[r] % ppr && prev_cuts[r] != P)) {
                set_error("bsmr_plan_shard_rebalance: previous cuts are not row-block boundaries");
                return BSMR_ERR_INVALID;
            }
            const u32 b0 = prev_cuts[r] / ppr, b1 = std::min(nRB, (prev_cuts[r + 1] + ppr - 1) / ppr);
            double pred = 0.0;
            for (u32 b = b0; b < b1; ++b) pred += block_cost[b];
            if (pred <= 0.0 || !(shard_ms[r] > 0.0f) || !std::isfinite(shard_ms[r])) continue;
            const double f = static_cast<double>(shard_ms[r]) / pred;
            for (u32 b = b0; b < b1; ++b) {
                scale[b] = f;
                measured[b] = 1;
            }
        }
        // normalise the factors of measured blocks to their mean; unmeasured blocks (a shard
        // whose time is 0 / NaN / inf) take the mean factor, i.e. keep their model cost
        double fs = 0.0;
        u32 nf = 0;
        for (u32 b = 0; b < nRB; ++b)
            if (measured[b]) {
                fs += scale[b];
                ++nf;
            }
        norm = nf ? fs / nf : 1.0;
        for (u32 b = 0; b < nRB; ++b)
            if (!measured[b]) scale[b] = norm;
    }
    std::vector<double> cum(nRB + 1ull, 0.0);
    for (u32 b = 0; b < nRB; ++b) cum[b + 1] = cum[b] + block_cost[b] * (scale[b] / norm);
    cut_row_blocks(cum, nRB, ppr, P, world, cuts);
    return BSMR_OK;
}

// the SpMM gather lists over caller arrays (spmm_schedule.cpp; no plan, no device)
extern "C" int bsmr_spmm_lists(uint32_t M, uint32_t N, uint32_t nnz, const uint32_t* rowptr,
                               const uint32_t* colidx, int side, uint32_t chunk, const uint32_t* order,
                               uint32_t norder, bsmr_spmm_seg* segs, uint64_t* nsegs, uint32_t* src,
                               uint32_t* vpos) {
    static_assert(sizeof(bsmr_spmm_seg) == sizeof(SpmmSeg), "bsmr_spmm_seg mirrors SpmmSeg");
    if (!rowptr || (nnz && !colidx) || !nsegs || (segs && nnz && (!src || !vpos))) {
        set_error("bsmr_spmm_lists: null argument");
        return BSMR_ERR_INVALID;
    }
    SpmmIn in;
    in.M = M;
    in.N = N;
    in.nnz = nnz;
    in.rowptr = rowptr;
    in.colidx = colidx;
    in.side = side;
    in.chunk = chunk;
    in.order = order;
    in.norder = order ? norder : 0;
    SpmmLists L;
    std::string err;
    if (spmm_lists(in, L, err, segs == nullptr)) {
        set_error("bsmr_spmm_lists: " + err);
        return BSMR_ERR_INVALID;
    }
    *nsegs = L.nSegs;
    if (!segs) return BSMR_OK;
    for (size_t i = 0; i < L.segs.size(); ++i)
        segs[i] = bsmr_spmm_seg{L.segs[i].dst, L.segs[i].first, L.segs[i].count, L.segs[i].part};
    std::copy(L.src.begin(), L.src.end(), src);
    std::copy(L.vpos.begin(), L.vpos.end(), vpos);
    return BSMR_OK;
}

// the row softmax's item list over a caller's rowptr (softmax_schedule.cpp; no plan, no device)
extern "C" int bsmr_softmax_items(uint32_t M, const uint32_t* rowptr, bsmr_softmax_item* items,
                                  uint64_t* nitems) {
    static_assert(sizeof(bsmr_softmax_item) == sizeof(SoftmaxItem), "bsmr_softmax_item mirrors SoftmaxItem");
    static_assert(BSMR_SOFTMAX_WAVE == SOFTMAX_WAVE && BSMR_SOFTMAX_BLOCK == SOFTMAX_BLOCK, "item kinds");
    if (!rowptr || !nitems) {
        set_error("bsmr_softmax_items: null argument");
        return BSMR_ERR_INVALID;
    }
    SoftmaxItems L;
    std::string err;
    if (softmax_items(M, rowptr, L, err, items == nullptr)) {
        set_error("bsmr_softmax_items: " + err);
        return BSMR_ERR_INVALID;
    }
    *nitems = L.nItems;
    for (size_t i = 0; items && i < L.items.size(); ++i)
        items[i] = bsmr_softmax_item{L.items[i].row, L.items[i].first, L.items[i].count, L.items[i].kind};
    return BSMR_OK;
}

extern "C" void bsmr_softmax_limits(uint32_t* wave_max, uint32_t* block_pass) {
    if (wave_max) *wave_max = SOFTMAX_WAVE_MAX;
    if (block_pass) *block_pass = SOFTMAX_BLOCK_PASS;
}

extern "C" int bsmr_plan_shard_rebalance(const bsmr_plan* plan, uint32_t K, int dtype, int world,
                                         const uint32_t* prev_cuts, const float* shard_ms,
                                         uint32_t* cuts) {
    if (!plan || world <= 0 || !prev_cuts || !shard_ms || !cuts || K == 0 || K % 16 ||
        (dtype != BSMR_F32 && dtype != BSMR_F16 && dtype != BSMR_BF16)) {
        set_error("bsmr_plan_shard_rebalance: bad arguments");
        return BSMR_ERR_INVALID;
    }
    const Plan& p = plan->p;
    const Plan::RowBlockLayout* L = nullptr;
    BSMR_CHECK(whole_rb_layout(p, K, dtype, &L, true));
    if (!L || L->nRB == 0 || L->orig) {
        set_error("bsmr_plan_shard_rebalance: needs the row-block launch of the reordered plan");
        return BSMR_ERR_UNSUPPORTED;
    }
    return bsmr_cost_cuts(L->rbCost.data(), L->nRB, L->RB / 16, p.P, world, prev_cuts, shard_ms, cuts);
}

extern "C" int bsmr_plan_shard_dtype(const bsmr_plan* plan, uint32_t K, int dtype, int rank,
                                     int world, uint32_t* p0, uint32_t* p1) {
    if (!plan || world <= 0 || rank < 0 || rank >= world || !p0 || !p1 || K == 0 || K % 16 ||
        (dtype != BSMR_F32 && dtype != BSMR_F16 && dtype != BSMR_BF16)) {
        set_error("bsmr_plan_shard: bad arguments");
        return BSMR_ERR_INVALID;
    }
    const Plan& p = plan->p;
    std::vector<u32> cuts(world + 1);
    // row-block launches: cut at row-block boundaries of the whole plan's layout by its measured
    // item costs (entries, column-run pieces, tiles, staged rows), so each shard's own layout has
    // the same row blocks; otherwise the per-panel model of bsmr_shard_cuts
    const Plan::RowBlockLayout* L = nullptr;
    BSMR_CHECK(whole_rb_layout(p, K, dtype, &L, true));
    if (L && L->nRB > 0 && !L->orig) {  // (original-order row blocks do not map to panels)
        BSMR_CHECK(bsmr_cost_cuts(L->rbCost.data(), L->nRB, L->RB / 16, p.P, world, nullptr, nullptr,
                                  cuts.data()));
    } else {
        BSMR_CHECK(bsmr_shard_cuts(p.h_blockOffsets.data(), p.h_sparseValueOffsets.data(), p.P, K,
                                   world, cuts.data()));
    }
    *p0 = cuts[rank];
    *p1 = cuts[rank + 1];
    return BSMR_OK;
}

namespace {
constexpr uint32_t RB_GEOM_WORDS = 13;

// the knobs of tuning t (null: defaults)
Knobs debug_knobs(const bsmr_tuning* t) {
    Knobs k;
    if (t) apply_tuning(k, *t);
    return k;
}
}  // namespace

// debug: the row-block geometry (rb_schedule.hpp rb_geometry) of rows of rowBytes over Rs staged
// rows holding n0 entries, NS gathered columns, a plan of nnz entries, original-order (orig) or
// column (cols) blocks, under tuning t (null: defaults) on a device of cus compute units. Needs no
// device. out[13] = {rowBytes, orig, cols, RB, NT, nRB, lds bytes, l2Kb, m, stagedWanted, staged,
// outCap, perBucket}. Not in the header (tests/test_rb_schedule_cpu.py)
extern "C" int bsmr_debug_rb_geometry(uint32_t rowBytes, uint32_t Rs, uint32_t n0, uint32_t NS,
                                      uint32_t nnz, int orig, int cols, const bsmr_tuning* t, int cus,
                                      uint32_t* out) {
    if (!out || rowBytes == 0 || cus <= 0 || NS > (1u << 22)) return BSMR_ERR_INVALID;
    const RbGeometry g = rb_geometry(rowBytes, Rs, n0, NS, nnz, cus, orig && !cols, cols != 0, debug_knobs(t));
    const uint32_t w[RB_GEOM_WORDS] = {g.rowBytes, g.orig, g.cols, g.RB, g.NT, g.nRB, static_cast<uint32_t>(g.lds),
                                       g.l2Kb, g.m, g.stagedWanted, g.staged, g.outCap, g.perBucket};
    std::copy(w, w + RB_GEOM_WORDS, out);
    return BSMR_OK;
}

// debug: the host-only scheduler (rb_schedule.hpp rb_schedule) on n entries given by their sorted
// columns (by row block, then column), rbEnd[nRB], the per-block kept-tile prefix keptBegin[nRB +
// 1] (null: no kept tiles), the geometry words of bsmr_debug_rb_geometry and tuning t (null:
// defaults); threads = host threads (0: the library's choice; the result does not depend on it).
// Needs no device. host_out = {n items, p pieces, items (4 u32 each), item ends, pieces (2 u32
// each), itemStat (4 u32 each), dynamic batches, work items}: *len = 4 + 9 n + 2 p; call with
// host_out = null for the length. Not in the header (tests/test_rb_schedule_cpu.py)
extern "C" int bsmr_debug_rb_schedule(const uint32_t* sorted_cols, uint64_t n, const uint32_t* rbEnd,
                                      const uint32_t* keptBegin, uint32_t NS, const uint32_t* geom,
                                      const bsmr_tuning* t, int threads, uint32_t* host_out,
                                      uint64_t* len) {
    if (!geom || !rbEnd || (n && !sorted_cols) || !len || threads < 0 || n > 0xffffffffull)
        return BSMR_ERR_INVALID;
    RbScheduleIn in;
    RbGeometry& g = in.geom;
    g.rowBytes = geom[0];
    g.orig = geom[1];
    g.cols = geom[2];
    g.RB = geom[3];
    g.NT = geom[4];
    g.nRB = geom[5];
    g.lds = geom[6];
    g.l2Kb = geom[7];
    g.m = geom[8];
    g.stagedWanted = geom[9];
    g.staged = geom[10];
    g.outCap = geom[11];
    g.perBucket = geom[12];
    if (g.nRB == 0 || g.m == 0 || g.perBucket == 0 || g.NT == 0 || g.RB == 0 || rbEnd[g.nRB - 1] != n)
        return BSMR_ERR_INVALID;
    in.entries = sorted_cols;
    in.n = n;
    in.rbEnd = rbEnd;
    in.keptBegin = keptBegin;
    in.NS = NS;
    const Knobs k = debug_knobs(t);
    in.knobs = &k;
    in.threads = static_cast<unsigned>(threads);
    RbScheduleOut o;
    rb_schedule(in, o);
    const uint64_t ni = o.items.size(), np = o.pieces.size();
    *len = 4 + 9 * ni + 2 * np;
    if (!host_out) return BSMR_OK;
    uint32_t* w = host_out;
    *w++ = static_cast<uint32_t>(ni);
    *w++ = static_cast<uint32_t>(np);
    for (const RbItem& it : o.items) { *w++ = it.x; *w++ = it.y; *w++ = it.z; *w++ = it.w; }
    for (uint32_t e : o.ends) *w++ = e;
    for (const RbPiece& pc : o.pieces) { *w++ = pc.x; *w++ = pc.y; }
    for (const RbItem& it : o.itemStat) { *w++ = it.x; *w++ = it.y; *w++ = it.z; *w++ = it.w; }
    *w++ = o.dyn;
    *w++ = o.nWorkItems;
    return BSMR_OK;
}

// debug: the host-only run cutting of staged output (rb_schedule.hpp rb_cut_runs) on nItems items
// given as ient = {first entry, entries} (2 u32 each) over sortedPos (every item's positions in
// ascending order), for a workgroup of NT threads; threads as above. Needs no device. host_out =
// {fits, n items, r runs, itemRuns (2 u32 each: first run, runs), runs (2 u32 each: position, slot |
// length << 16)} with r = 0 when the table does not fit: *len = 3 + 2 n + 2 r; call with host_out =
// null for the length. Not in the header (tests/test_store_ref_cpu.py)
extern "C" int bsmr_debug_rb_runs(const uint32_t* sortedPos, uint64_t nPos, const uint32_t* ient,
                                  uint64_t nItems, uint32_t NT, int threads, uint32_t* host_out,
                                  uint64_t* len) {
    if ((nPos && !sortedPos) || (nItems && !ient) || !len || NT == 0 || threads < 0 || nPos > 0xffffffffull)
        return BSMR_ERR_INVALID;
    for (uint64_t i = 0; i < nItems; ++i)
        if (static_cast<uint64_t>(ient[2 * i]) + ient[2 * i + 1] > nPos || ient[2 * i + 1] > 65535u)
            return BSMR_ERR_INVALID;
    std::vector<RbPiece> ie(nItems);
    for (uint64_t i = 0; i < nItems; ++i) ie[i] = RbPiece{ient[2 * i], ient[2 * i + 1]};
    RbRuns rr;
    rb_cut_runs(sortedPos, ie.data(), nItems, NT, rr, static_cast<unsigned>(threads));
    *len = 3 + 2 * nItems + 2 * rr.runs.size();
    if (!host_out) return BSMR_OK;
    uint32_t* w = host_out;
    *w++ = rr.fits;
    *w++ = static_cast<uint32_t>(nItems);
    *w++ = static_cast<uint32_t>(rr.runs.size());
    for (const RbPiece& r : rr.itemRuns) { *w++ = r.x; *w++ = r.y; }
    for (const RbPiece& r : rr.runs) { *w++ = r.x; *w++ = r.y; }
    return BSMR_OK;
}

namespace {
void put_choice(const LaunchChoice& c, uint32_t* out) {
    out[0] = static_cast<uint32_t>(c.kind);
    out[1] = static_cast<uint32_t>(c.slot + 1);
    out[2] = c.rowBytes;
}
void put_form(const RbForm& f, uint32_t* out) {
    const uint32_t w[9] = {f.stageNt, f.lateB, f.pairs, f.lite, f.dyn, f.NT, f.grid, f.ldsBytes, f.stageBlocks};
    std::copy(w, w + 9, out);
}
}  // namespace

// debug: the launch (launch_select.hpp choose_launch) of a plan with facts = {M, N, nnz, residual
// entries, dense tiles}, layout auto (layout_rowblock 1, force_rowblock 0), row-block (1, 1) or
// column-major (0, 0), under tuning t (null: defaults). Needs no device. out[3] = {kind (0 panel
// tile, 1 dense-sampled, 2 row-block, 3 column-major half, 4 column-major fp32), row-block slot +
// 1 (0: none), row bytes}; returns the status of the K / dtype rules (validate_kd, then the chosen
// launch's validate_launch_k), their text in bsmr_last_error. Not in the header
// (tests/test_launch_select_cpu.py)
extern "C" int bsmr_debug_launch_choice(const uint32_t* facts, int layout_rowblock, int force_rowblock,
                                        const bsmr_tuning* t, uint32_t K, int dtype, uint32_t* out) {
    if (!facts || !out) return BSMR_ERR_INVALID;
    Knobs k = debug_knobs(t);
    k.use_rowblock = layout_rowblock != 0;
    k.force_rowblock = force_rowblock != 0;
    const LaunchChoice c = choose_launch({facts[0], facts[1], facts[2], facts[3], facts[4]}, k, K, dtype);
    put_choice(c, out);
    BSMR_CHECK(report(validate_kd("bsmr_debug_launch_choice", K, dtype)));
    return report(validate_launch_k("bsmr_debug_launch_choice", c.kind, K));
}

// debug: whether a plan of facts[0] = M rows and facts[1] = N columns with bsmr_tuning.col_blocks =
// col_blocks builds the column-block candidate for rows of rowBytes (launch_select.hpp
// col_block_candidate): 1 or 0, -1 without facts. Needs no device. Not in the header
// (tests/test_launch_select_cpu.py)
extern "C" int bsmr_debug_col_block_candidate(const uint32_t* facts, int col_blocks, uint32_t rowBytes) {
    if (!facts) return -1;
    PlanFacts f;
    f.M = facts[0];
    f.N = facts[1];
    Knobs k;
    k.col_blocks = col_blocks;  // (as given: not through apply_tuning's clamp)
    return col_block_candidate(f, k, rowBytes) ? 1 : 0;
}

// debug: the panel-range rules (launch_select.hpp check_panel_range) as entry point `who` reports
// them for a plan of P panels whose (K, dtype) has row-block slot `slot` (-1: none): the status,
// its text in bsmr_last_error. Needs no device. Not in the header
extern "C" int bsmr_debug_panel_range(const char* who, uint32_t p0, uint32_t p1, uint32_t P, int slot,
                                      int dtype, int local) {
    if (!who) return BSMR_ERR_INVALID;
    return report(check_panel_range(who, p0, p1, P, slot, dtype, local != 0));
}

// debug: the form (launch_select.hpp rb_form) of a row-block launch of mode (1 tiles, 2 residual, 3
// both) over a layout with layoutFacts = {rowBytes, NT, nItems, nTilesKept, outLds, outRuns,
// dynBatches} under tuning t (null: defaults). Needs no device. out[9] = {stageNt, lateB, pairs,
// lite, dyn, NT, grid, LDS bytes, stageBlocks (0: the A image's)}. Not in the header
extern "C" int bsmr_debug_rb_form(const uint32_t* layoutFacts, const bsmr_tuning* t, uint32_t mode,
                                  uint32_t* out) {
    if (!layoutFacts || !out) return BSMR_ERR_INVALID;
    const uint32_t* w = layoutFacts;
    put_form(rb_form({w[0], w[1], w[2], w[3], w[4], w[5] != 0, w[6] != 0}, debug_knobs(t), mode), out);
    return BSMR_OK;
}

// debug: what bsmr_sddmm runs on this plan for (K, dtype): out[13] = the three words of
// bsmr_debug_launch_choice, then for the row-block kind the nine of bsmr_debug_rb_form for the
// whole launch of the plan's layout (built on first use, as bsmr_debug_rb_items does; else
// zeros) and whether that layout's output is packed (the CSR position in the metadata's low 22
// bits, no `out` array). Not in the header (tests/sddmm_cases.py)
extern "C" int bsmr_debug_plan_launch(const bsmr_plan* plan, uint32_t K, int dtype, uint32_t* out) {
    if (!plan || !out) return BSMR_ERR_INVALID;
    BSMR_CHECK(report(validate_kd("bsmr_debug_plan_launch", K, dtype)));
    const Plan& p = plan->p;
    const LaunchChoice c = choose_launch(p, K, dtype);
    std::fill(out, out + 13, 0u);
    put_choice(c, out);
    if (c.kind != Launch::RowBlock) return BSMR_OK;
    const Plan::RowBlockLayout* L = nullptr;
    BSMR_CHECK(whole_rb_layout(p, K, dtype, &L));
    put_form(rb_form(rb_layout_facts(*L), p.k, 3), out + 3);
    out[12] = L->outPacked ? 1u : 0u;
    return BSMR_OK;
}
