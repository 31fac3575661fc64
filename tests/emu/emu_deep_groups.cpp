// Host emulation of the evaluation kernels behind include/bfstark_open.h (csrc/deep.hip over csrc/deep_core.hpp): separate columns of
// different lengths in one simulated launch -- with the launch's own layout of partial sums, painted so that a slot no workgroup wrote
// shows if the combining step reads it.  The quotient of an opening plan is emulated beside the quotient across commitments, by the
// same driver (emu_deep_rounds.cpp).  TEST INFRASTRUCTURE, see emu_ntt.cpp.
#include <vector>

#include "../../stark_brainfuck_amd/csrc/deep_core.hpp"

using namespace bfs;

extern "C" unsigned emu_deep_groups_share(unsigned n_points) { return DEEP_G_T * deep_groups_e(n_points); }

namespace {

constexpr u64 UNWRITTEN = 0xFFFFFFFFDEADBEEFull;          // not a residue: xfe arithmetic on it trips BFS_CHECK_CANONICAL or gives a wrong sum

template <int K>
void eval_columns_k(const DeepEvalColumns& cols, u32 count, const u64* table, u64* out) {
    u32 row_blocks = 0;
    for (u32 b = 0; b < count; ++b) row_blocks = deep_eval_blocks(cols.n[b]) > row_blocks ? deep_eval_blocks(cols.n[b]) : row_blocks;
    std::vector<u64> partial((size_t)count * K * row_blocks * 3, UNWRITTEN);
    for (u32 b = 0; b < count; ++b)                       // launch 1: grid (row_blocks, count)
        for (u32 block = 0; block < row_blocks; ++block) {
            if (block >= deep_eval_blocks(cols.n[b])) continue;
            Xfe sum[K];
            for (int j = 0; j < K; ++j) sum[j] = Xfe{{0, 0, 0}};
            for (u32 t = 0; t < DEEP_EVAL_T; ++t) {
                Xfe mine[K];
                deep_eval_thread<K>(cols.col[b], cols.n[b], block, t, table + DEEP_EVAL_STEPS_AT, table, mine);
                for (int j = 0; j < K; ++j) sum[j] = xfe_add(sum[j], mine[j]);
            }
            for (int j = 0; j < K; ++j)
                for (int l = 0; l < 3; ++l) partial[deep_eval_partial_at(b, K, j, row_blocks, block) + l] = sum[j].c[l];
        }
    for (u32 b = 0; b < count; ++b)                       // launch 2: block b * K + j
        for (int j = 0; j < K; ++j) {
            Xfe total{{0, 0, 0}};
            const Xfe zb = deep_eval_block_power(table, j);
            for (u32 p = 0; p < deep_eval_blocks(cols.n[b]); ++p)
                total = xfe_add(total, xfe_mul(xfe_load3(partial.data() + deep_eval_partial_at(b, K, j, row_blocks, 0) + (size_t)p * 3), xfe_pow_small(zb, p)));
            for (int l = 0; l < 3; ++l) out[((u64)b * K + j) * 3 + l] = total.c[l];
        }
}

}  // namespace

// bfsx_poly_eval_columns as the launches compute it; -1: arguments the entry point refuses
extern "C" int emu_deep_eval_columns(const u64* const* columns, const u64* lengths, unsigned count, const u64* points, unsigned k, u64* out) {
    if (count < 1 || count > DEEP_EVAL_MAX_COLUMNS || k < 1 || k > DEEP_MAX_POINTS) return -1;
    DeepEvalColumns cols{};
    for (u32 b = 0; b < count; ++b) {
        if (lengths[b] < 1 || lengths[b] > (1ull << 24)) return -1;
        cols.col[b] = columns[b];
        cols.n[b] = (u32)lengths[b];
    }
    std::vector<u64> table(DEEP_EVAL_TABLE_WORDS, 0);
    for (u32 j = 0; j < k; ++j)
        for (u32 t = 0; t < DEEP_EVAL_T; ++t) deep_eval_table_entry(xfe_load3(points + 3 * j), j, t, table.data());
    return deep_with_count<DEEP_MAX_POINTS>(k, [&](auto kk) { eval_columns_k<decltype(kk)::value>(cols, count, table.data(), out); return 0; });
}
