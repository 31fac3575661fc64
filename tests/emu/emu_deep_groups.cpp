// Host emulation of the kernels behind include/bfstark_open.h (csrc/deep.hip over csrc/deep_core.hpp): evaluation of separate columns of
// different lengths in one simulated launch -- with the launch's own layout of partial sums, painted so that a slot no workgroup wrote
// shows if the combining step reads it -- and the quotient of an opening plan, every thread of every workgroup running the kernel's
// per-thread code.  TEST INFRASTRUCTURE, see emu_ntt.cpp.
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

template <int NP>
void groups_np(const DeepGroupsArgs& a, u64* out, u64 out_stride) {
    constexpr int E = (int)deep_groups_e(NP);
    const u64 per_block = (u64)DEEP_G_T * E;
    for (u64 block = 0; block * per_block < a.n; ++block)
        for (u32 t = 0; t < DEEP_G_T; ++t) {
            u64 idx[E];
            for (int e = 0; e < E; ++e) idx[e] = block * per_block + (u64)e * DEEP_G_T + t;
            Xfe g[E];
            deep_groups_thread<NP, E>(a, idx, g);
            for (int e = 0; e < E; ++e)
                if (idx[e] < a.n)
                    for (int l = 0; l < 3; ++l) out[(u64)l * out_stride + idx[e]] = g[e].c[l];
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
    switch (k) {
    case 1: eval_columns_k<1>(cols, count, table.data(), out); break;
    case 2: eval_columns_k<2>(cols, count, table.data(), out); break;
    case 3: eval_columns_k<3>(cols, count, table.data(), out); break;
    default: eval_columns_k<4>(cols, count, table.data(), out); break;
    }
    return 0;
}

// bfsx_deep_quotient_groups as the launch computes it.  columns[c]: the codeword's first word, IN GROUP ORDER; is_ext[c]
extern "C" int emu_deep_quotient_groups(const u64* const* columns, const int* is_ext, unsigned m, u64 limb_stride, unsigned log_n, u64 offset, u64 omega,
                                        const unsigned* group_columns, const unsigned* group_pairs, unsigned n_groups, const u64* points,
                                        unsigned n_points, const unsigned* pair_point, const u64* pair_values, const u64* lambda, u64* out, u64 out_stride) {
    if (m < 1 || m > DEEP_MAX_COLUMNS || n_groups < 1 || n_groups > DEEP_G_GROUPS || n_points < 1 || n_points > DEEP_G_POINTS || log_n < 1 || log_n > 24) return -1;
    DeepGroupsArgs a{};
    a.n_groups = n_groups; a.limb_stride = limb_stride; a.n = 1ull << log_n; a.offset = offset;
    for (u32 p = 0; p < n_points; ++p) deep_group_point(a.pt[p], xfe_load3(points + 3 * p));
    const Xfe lam = xfe_load3(lambda);
    u32 c = 0, q = 0;
    Xfe scale{{1, 0, 0}};
    for (u32 g = 0; g < n_groups; ++g) {
        if (group_columns[g] < 1 || c + group_columns[g] > m || group_pairs[g] < 1 || group_pairs[g] > DEEP_MAX_POINTS || q + group_pairs[g] > DEEP_G_PAIRS) return -1;
        Xfe power{{1, 0, 0}};
        for (u32 r = 0; r < group_columns[g]; ++r, ++c) {
            a.col[c] = columns[c];
            if (is_ext[c]) a.ext_mask |= 1u << c;
            lazy_weight_matrix(power, a.weight[c]);
            power = xfe_mul(power, lam);
        }
        for (u32 j = 0; j < group_pairs[g]; ++j, ++q) {
            if (pair_point[q] >= n_points) return -1;
            DeepGroupPair& pr = a.pair[q];
            pr.scale = scale; pr.y = xfe_load3(pair_values + 3 * q); pr.point = pair_point[q];
            pr.unit = scale.c[0] == 1 && scale.c[1] == 0 && scale.c[2] == 0;
            scale = xfe_mul(scale, power);
        }
        a.col_end[g] = c; a.pair_end[g] = q;
    }
    if (c != m) return -1;
    a.lo_bits = (log_n + 1) / 2;                          // the two-level table of the launch
    std::vector<u64> lo(1ull << a.lo_bits), hi(1ull << (log_n - a.lo_bits));
    for (u64 i = 0; i < lo.size(); ++i) lo[i] = gl_pow(omega, i);
    for (u64 i = 0; i < hi.size(); ++i) hi[i] = gl_pow(omega, i << a.lo_bits);
    a.w_lo = lo.data(); a.w_hi = hi.data();
    switch (n_points) {
    case 1: groups_np<1>(a, out, out_stride); break;
    case 2: groups_np<2>(a, out, out_stride); break;
    case 3: groups_np<3>(a, out, out_stride); break;
    case 4: groups_np<4>(a, out, out_stride); break;
    case 5: groups_np<5>(a, out, out_stride); break;
    case 6: groups_np<6>(a, out, out_stride); break;
    case 7: groups_np<7>(a, out, out_stride); break;
    default: groups_np<8>(a, out, out_stride); break;
    }
    return 0;
}
