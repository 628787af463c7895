// spmm_panels.hpp — what the panel form of SpMM (bsmr_spmm_panels / bsmr_spmm_t_panels,
// spmm_panels.hip) adds on the host to the panel lists of attention_panels.hpp: where in the
// caller's V the entry behind every set mask bit lies. Standard library only: no HIP, no device.
//
// The lists themselves are the attention forward's (rows side: attention_panel_lists over the
// plan's row order) and the panel backward's (columns side: the same call on the transposed
// pattern). A CSR row's columns are in file order here, not sorted, so the position of an entry
// cannot be derived from the row pointer and a popcount over the CSR: it is listed. pos holds one
// u32 per stored entry, ordered step by step, panel row by panel row, mask bit by mask bit; base
// holds 16 u32 per step, and the entry of (step s, panel row r, slot c) is
//   V[pos[base[16 s + r] + popcount(masks[r] & ((1 << c) - 1))]].
// Padding slots and unset bits have no entry. 4 bytes per stored entry and 64 per step: a dense
// 16 x 32 position tile per step would be ten times that at a fill of 94 permille.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "attention_panels.hpp"

namespace bsmr {

// The pattern of S^T as attention_pattern_transpose gives it, and with it tpos: the CSR index in S
// of every entry of the transposed CSR (what carries an entry's place in V to the columns side).
// 0, or 1 with `err` set (the transpose's rules).
int spmm_pattern_transpose_pos(uint32_t M, uint32_t N, const uint32_t* rowptr, const uint32_t* colidx,
                               std::vector<uint32_t>& trowptr, std::vector<uint32_t>& tcolidx, std::vector<uint32_t>& tpos,
                               std::string& err);

// base (16 per step) and pos (one per entry) of the lists `rows` / `steps` / `items` built from the
// CSR (M, N, rowptr, colidx); entry e of that CSR lies at V[epos[e]] (epos null: at V[e]). 0, or 1
// with `err` set: a null pointer, a rowptr not ascending from 0, an item, row or step out of
// range, or a mask bit whose (row, column) the CSR does not store exactly once (lists of another
// pattern).
int spmm_panel_positions(uint32_t M, uint32_t N, const uint32_t* rowptr, const uint32_t* colidx, const uint32_t* epos,
                         const uint32_t* rows, const PanelStep* steps, uint64_t nsteps, const PanelItem* items, uint64_t nitems,
                         std::vector<uint32_t>& base, std::vector<uint32_t>& pos, std::string& err);

}  // namespace bsmr
