// Stand-alone driver of the host-only layout rules of the strided attention operands
// (csrc/attention_layout.cpp), built by tests/test_attention_layout_cpu.py under
// -fsanitize=address,undefined. Reads a table file, one case per line:
//   "<ptr> <batch> <head> <row> <batches> <heads> <rows> <width> <elem_bytes> <is_output>"
// (decimal; the word "null" for ptr is the null operand) and prints one line per case: "0" when
// every rule holds, else "1 <the rule>", for the test to compare with the library's answer.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>

#include "attention_layout.hpp"

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <table file>\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    char ptr[64];
    uint64_t batch, head, row;
    uint32_t batches, heads, rows, width, esz, out;
    int n;
    while ((n = fscanf(f, "%63s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32
                          " %" SCNu32 " %" SCNu32,
                       ptr, &batch, &head, &row, &batches, &heads, &rows, &width, &esz, &out)) == 10) {
        bsmr_attention_operand op;
        const bool null = strcmp(ptr, "null") == 0;
        op.ptr = reinterpret_cast<void*>(static_cast<uintptr_t>(null ? 0 : strtoull(ptr, nullptr, 10)));
        op.batch = batch;
        op.head = head;
        op.row = row;
        std::string err;
        const int st = bsmr::attention_layout_check(null ? nullptr : &op, batches, heads, rows, width, esz, out != 0, err);
        if (st != 0 && st != 1) return 3;
        if ((st == 0) != err.empty()) return 3;  // a message exactly when a rule fails
        if (st)
            printf("1 %s\n", err.c_str());
        else
            printf("0\n");
    }
    fclose(f);
    return n == EOF ? 0 : 2;
}
