// Stand-alone driver of csrc/attention_panels.cpp for tests/test_attention_panels_cpu.py (built under
// -fsanitize=address,undefined). Reads "M N norder", rowptr, colidx and order (decimal) and prints
// each list as one line of numbers ("rows", "steps", "items", "reds"), or "error <message>".
#include <cinttypes>
#include <cstdio>
#include <string>
#include <vector>

#include "attention_panels.hpp"

static bool read(FILE* f, std::vector<uint32_t>& v, size_t n) {
    v.resize(n);
    for (size_t i = 0; i < n; ++i)
        if (fscanf(f, "%" SCNu32, &v[i]) != 1) return false;
    return true;
}

int main(int argc, char** argv) {
    FILE* f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    uint32_t M, N, norder;
    std::vector<uint32_t> rp, ci, order;
    if (!f || fscanf(f, "%" SCNu32 " %" SCNu32 " %" SCNu32, &M, &N, &norder) != 3 || !read(f, rp, M + 1) ||
        !read(f, ci, rp[M]) || !read(f, order, norder))
        return 2;
    fclose(f);
    bsmr::PanelLists L;
    std::string err;
    if (bsmr::attention_panel_lists(M, N, rp.data(), ci.data(), order.data(), norder, L, err)) {
        printf("error %s\n", err.c_str());
        return 0;
    }
    if (L.steps.size() != L.nSteps || L.items.size() != L.nItems || L.reds.size() != L.splitPanels) return 3;
    printf("rows");
    for (uint32_t r : L.rows) printf(" %" PRIu32, r);
    printf("\nsteps");
    for (const bsmr::PanelStep& s : L.steps) {
        for (uint32_t c : s.cols) printf(" %" PRIu32, c);
        for (uint32_t m : s.masks) printf(" %" PRIu32, m);
    }
    printf("\nitems");
    for (const bsmr::PanelItem& i : L.items) printf(" %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32, i.row0, i.step0, i.nsteps, i.part);
    printf("\nreds");
    for (const bsmr::PanelRed& r : L.reds) printf(" %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32, r.row0, r.part0, r.nparts, r.pad);
    printf("\n");
    return 0;
}
