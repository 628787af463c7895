// attention_layout.hpp — the layout rules of a strided attention operand
// (bsmr_attention_operand, include/bsmr.h): host only, plain C++ without a HIP header, and the only
// place the rules are written. bsmr_attention_heads, bsmr_attention_backward_heads and
// bsmr_attention_layout_check all go through attention_layout_check.
#pragma once

#include <cstdint>
#include <string>

#include "bsmr.h"

namespace bsmr {

// Element [b][h][r][c] of the operand lies at ptr + (b batch + h head + r row + c) elements,
// b < batches, h < heads, r < rows, c < width; the last dimension is contiguous. A dimension of
// extent 1 is never stepped over and its stride is not looked at. Returns 0 and leaves `err` alone
// when every rule holds, else 1 with `err` naming the first rule that does not:
//   * op and op->ptr are non-null and ptr is 16-byte aligned; rows, width and elem_bytes are
//     positive; batches is 1 .. BSMR_ATTENTION_MAX_BATCHES and heads 1 .. BSMR_ATTENTION_MAX_HEADS;
//   * every stride times elem_bytes is a multiple of 16 bytes (computed without overflow);
//   * with more than one row, row >= width, and row times elem_bytes stays below 2^32 (the
//     kernels multiply a 32-bit row index by a 32-bit row stride in bytes);
//   * the offset of the last byte, ((batches - 1) batch + (heads - 1) head + (rows - 1) row +
//     width) elem_bytes, fits in 64 bits, and so does ptr plus that offset; every product and sum
//     is overflow-checked;
//   * an input may have a batch or head stride of 0 (one K / V shared by every head);
//   * an output must be provably non-overlapping: the dimensions among (batch, head, row) of
//     extent > 1, sorted by stride ascending, have a first stride >= width and every further
//     stride >= the previous stride times the previous extent. Dense (B, H, M, W), dense
//     (B, M, H, W) and their padded variants pass; a stride of 0 does not.
int attention_layout_check(const bsmr_attention_operand* op, uint32_t batches, uint32_t heads, uint32_t rows,
                           uint32_t width, uint32_t elem_bytes, bool is_output, std::string& err);

// The strides of a contiguous (batches, heads, rows, width) operand: what the single-slice entry
// points pass for their dense pointers
inline bsmr_attention_operand attention_dense_operand(const void* ptr, uint32_t heads, uint32_t rows, uint32_t width) {
    bsmr_attention_operand op;
    op.ptr = const_cast<void*>(ptr);
    op.row = width;
    op.head = static_cast<uint64_t>(rows) * width;
    op.batch = op.head * heads;
    return op;
}

}  // namespace bsmr
