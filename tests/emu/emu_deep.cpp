// Host emulation of the two kernels of csrc/deep.hip over csrc/deep_core.hpp: every thread of every workgroup of a simulated launch runs
// the kernel's per-thread code; the workgroup sums and the combining launch are plain field additions here as there (exact, so the
// order is immaterial).  TEST INFRASTRUCTURE, see emu_ntt.cpp.
#include <vector>

#include "../../stark_brainfuck_amd/csrc/deep_core.hpp"

using namespace bfs;

extern "C" unsigned emu_deep_eval_block(void) { return DEEP_EVAL_BLOCK; }
extern "C" unsigned emu_deep_eval_threads(void) { return DEEP_EVAL_T; }

template <int K>
static void eval_k(const u64* coeffs, u64 n, u64 in_stride, u32 batch, const u64* table, u64* out) {
    const u64 blocks = (n + DEEP_EVAL_BLOCK - 1) / DEEP_EVAL_BLOCK;
    for (u32 b = 0; b < batch; ++b) {
        Xfe total[K];
        for (int j = 0; j < K; ++j) total[j] = Xfe{{0, 0, 0}};
        for (u64 block = 0; block < blocks; ++block) {
            Xfe partial[K];
            for (int j = 0; j < K; ++j) partial[j] = Xfe{{0, 0, 0}};
            for (u32 t = 0; t < DEEP_EVAL_T; ++t) {
                Xfe mine[K];
                deep_eval_thread<K>(coeffs + (u64)b * in_stride, n, block, t, table + DEEP_EVAL_STEPS_AT, table, mine);
                for (int j = 0; j < K; ++j) partial[j] = xfe_add(partial[j], mine[j]);
            }
            for (int j = 0; j < K; ++j)      // the combining launch
                total[j] = xfe_add(total[j], xfe_mul(partial[j], xfe_pow_small(deep_eval_block_power(table, j), block)));
        }
        for (int j = 0; j < K; ++j)
            for (int l = 0; l < 3; ++l) out[((u64)b * K + j) * 3 + l] = total[j].c[l];
    }
}

// bfs_poly_eval_points as the launches compute it; -1: arguments the entry point refuses
extern "C" int emu_deep_eval(const u64* coeffs, u64 n, u64 in_stride, unsigned batch, const u64* points, unsigned k, u64* out) {
    if (n < 1 || n > (1ull << 24) || batch < 1 || k < 1 || k > DEEP_MAX_POINTS || (batch > 1 && in_stride < n)) return -1;
    std::vector<u64> table(DEEP_EVAL_TABLE_WORDS, 0);
    for (u32 j = 0; j < k; ++j)
        for (u32 t = 0; t < DEEP_EVAL_T; ++t) deep_eval_table_entry(Xfe{{points[3 * j], points[3 * j + 1], points[3 * j + 2]}}, j, t, table.data());
    return deep_with_count<DEEP_MAX_POINTS>(k, [&](auto kk) { eval_k<decltype(kk)::value>(coeffs, n, in_stride, batch, table.data(), out); return 0; });
}

template <int K>
static void quotient_k(const DeepQuotientArgs& a, u64* out, u64 out_stride) {
    const u64 per_block = (u64)DEEP_Q_T * DEEP_Q_E;
    for (u64 block = 0; block * per_block < a.n; ++block)
        for (u32 t = 0; t < DEEP_Q_T; ++t) {
            u64 idx[DEEP_Q_E];
            for (u32 e = 0; e < DEEP_Q_E; ++e) idx[e] = block * per_block + (u64)e * DEEP_Q_T + t;
            Xfe g[DEEP_Q_E];
            deep_quotient_thread<K>(a, idx, g);
            for (u32 e = 0; e < DEEP_Q_E; ++e)
                if (idx[e] < a.n)
                    for (int l = 0; l < 3; ++l) out[(u64)l * out_stride + idx[e]] = g[e].c[l];
        }
}

// bfs_deep_quotient as the launch computes it.  columns[p]: the codeword's first word; is_ext[p]; planes limb_stride apart
extern "C" int emu_deep_quotient(const u64* const* columns, const int* is_ext, unsigned m, u64 limb_stride, unsigned log_n, u64 offset, u64 omega,
                                 const u64* points, const u64* values, unsigned k, const u64* lambda, u64* out, u64 out_stride) {
    if (m < 1 || m > DEEP_MAX_COLUMNS || k < 1 || k > DEEP_MAX_POINTS || log_n < 1 || log_n > 24) return -1;
    DeepQuotientArgs a{};
    a.m = m; a.limb_stride = limb_stride; a.n = 1ull << log_n; a.offset = offset;
    const Xfe lam{{lambda[0], lambda[1], lambda[2]}};
    Xfe power{{1, 0, 0}};
    for (u32 p = 0; p < m; ++p) {
        a.col[p] = columns[p];
        if (is_ext[p]) a.ext_mask |= 1u << p;
        lazy_weight_matrix(power, a.weight[p]);
        power = xfe_mul(power, lam);
    }
    Xfe scale{{1, 0, 0}};
    for (u32 j = 0; j < k; ++j) {
        deep_point_consts(a.pt[j], Xfe{{points[3 * j], points[3 * j + 1], points[3 * j + 2]}}, scale, Xfe{{values[3 * j], values[3 * j + 1], values[3 * j + 2]}});
        scale = xfe_mul(scale, power);
    }
    std::vector<u64> omegas;
    deep_host_omega_tables(a, omega, log_n, omegas);
    return deep_with_count<DEEP_MAX_POINTS>(k, [&](auto kk) { quotient_k<decltype(kk)::value>(a, out, out_stride); return 0; });
}
