// attention_layout.cpp — the layout rules of a strided attention operand (attention_layout.hpp).
// Host only: plain C++, no HIP header, no device call.
#include "attention_layout.hpp"

#include <algorithm>

namespace bsmr {
namespace {

bool mul(uint64_t a, uint64_t b, uint64_t& out) { return !__builtin_mul_overflow(a, b, &out); }
bool add(uint64_t a, uint64_t b, uint64_t& out) { return !__builtin_add_overflow(a, b, &out); }

struct Dim {
    const char* name;
    uint64_t stride, extent;
};

}  // namespace

int attention_layout_check(const bsmr_attention_operand* op, uint32_t batches, uint32_t heads, uint32_t rows,
                           uint32_t width, uint32_t elem_bytes, bool is_output, std::string& err) {
    if (!op) {
        err = "null operand";
        return 1;
    }
    if (batches == 0 || batches > BSMR_ATTENTION_MAX_BATCHES || heads == 0 || heads > BSMR_ATTENTION_MAX_HEADS) {
        err = "batches must be 1 .. " + std::to_string(BSMR_ATTENTION_MAX_BATCHES) + " and heads 1 .. " +
              std::to_string(BSMR_ATTENTION_MAX_HEADS) + ", got " + std::to_string(batches) + " and " +
              std::to_string(heads);
        return 1;
    }
    if (rows == 0 || width == 0 || elem_bytes == 0) {
        err = "rows, width and element size must be positive";
        return 1;
    }
    if (!op->ptr) {
        err = "null device pointer";
        return 1;
    }
    if (reinterpret_cast<uintptr_t>(op->ptr) & 15u) {
        err = "pointer is not 16-byte aligned";
        return 1;
    }
    // the dimensions that are stepped over
    Dim dims[3];
    int nd = 0;
    if (batches > 1) dims[nd++] = Dim{"batch", op->batch, batches};
    if (heads > 1) dims[nd++] = Dim{"head", op->head, heads};
    if (rows > 1) dims[nd++] = Dim{"row", op->row, rows};
    uint64_t last = width;  // elements up to and including the last one
    for (int i = 0; i < nd; ++i) {
        const Dim& d = dims[i];
        uint64_t bytes, span;
        if (!mul(d.stride, elem_bytes, bytes)) {
            err = std::string(d.name) + " stride in bytes does not fit in 64 bits";
            return 1;
        }
        if (bytes & 15u) {
            err = std::string(d.name) + " stride of " + std::to_string(d.stride) + " elements is not a multiple of 16 bytes";
            return 1;
        }
        if (!mul(d.stride, d.extent - 1, span) || !add(last, span, last)) {
            err = "the offset of the last element does not fit in 64 bits";
            return 1;
        }
    }
    uint64_t lastBytes, end;
    if (!mul(last, elem_bytes, lastBytes) || !add(reinterpret_cast<uintptr_t>(op->ptr), lastBytes, end)) {
        err = "the offset of the last byte does not fit in 64 bits";
        return 1;
    }
    if (rows > 1) {
        if (op->row < width) {
            err = "row stride of " + std::to_string(op->row) + " elements is below the row width " + std::to_string(width);
            return 1;
        }
        if (op->row * elem_bytes >= (1ull << 32)) {  // (no overflow: checked above)
            err = "row stride of " + std::to_string(op->row) + " elements reaches 2^32 bytes";
            return 1;
        }
    }
    if (is_output) {
        std::stable_sort(dims, dims + nd, [](const Dim& a, const Dim& b) { return a.stride < b.stride; });
        uint64_t need = width;  // what the next stride must reach
        for (int i = 0; i < nd; ++i) {
            const Dim& d = dims[i];
            if (d.stride < need) {
                err = std::string("output may overlap itself: ") + d.name + " stride of " + std::to_string(d.stride) +
                      " elements is below " + std::to_string(need);
                return 1;
            }
            if (!mul(d.stride, d.extent, need)) {
                err = "the extent of an output dimension does not fit in 64 bits";
                return 1;
            }
        }
    }
    return 0;
}

}  // namespace bsmr
