// Host emulation of the launches behind both plan entries of csrc/deep.hip (include/bfstark_open.h: the quotient of an opening plan in
// one launch; include/bfstark_rounds.h: of a plan over the columns of several commitments), driven as the library drives them: the
// library's own check of the plan (deep_plan_check) against the entry's limits, its own split between launches (deep_rounds_split), its
// own arguments of every launch (deep_rounds_args), and every thread of every workgroup of every launch running the kernel's per-thread
// code -- the first launch from zero without reading the output, every later one from what the output holds.  TEST INFRASTRUCTURE, see
// emu_ntt.cpp.
#include <vector>

#include "../../stark_brainfuck_amd/csrc/deep_core.hpp"

using namespace bfs;

namespace {

template <int NP, bool ACC>
void launch_np(const DeepGroupsArgs& a, u64* out, u64 out_stride) {
    constexpr int E = (int)deep_groups_e(NP);
    const u64 per_block = (u64)DEEP_G_T * E;
    for (u64 block = 0; block * per_block < a.n; ++block)
        for (u32 t = 0; t < DEEP_G_T; ++t) {
            u64 idx[E];
            for (int e = 0; e < E; ++e) idx[e] = block * per_block + (u64)e * DEEP_G_T + t;
            Xfe g[E];
            if (ACC) {
                Xfe start[E];
                for (int e = 0; e < E; ++e) {
                    const u64 at = idx[e] < a.n ? idx[e] : 0;
                    start[e] = Xfe{{out[at], out[out_stride + at], out[2 * out_stride + at]}};
                }
                deep_groups_thread_from<NP, E>(a, idx, start, g);
            } else {
                deep_groups_thread<NP, E>(a, idx, g);
            }
            for (int e = 0; e < E; ++e)
                if (idx[e] < a.n)
                    for (int l = 0; l < 3; ++l) out[(u64)l * out_stride + idx[e]] = g[e].c[l];
        }
}

// deep.hip's deep_quotient_plan on host memory.  -> the number of launches, -1: arguments the entry refuses
int plan_quotient(const DeepPlanLimits& limits, const u64* const* columns, const int* is_ext, unsigned m, u64 limb_stride, unsigned log_n, u64 offset,
                  u64 omega, const unsigned* group_columns, const unsigned* group_pairs, unsigned n_groups, const u64* points, unsigned n_points,
                  const unsigned* pair_point, const u64* pair_values, const u64* lambda, u64* out, u64 out_stride) {
    char why[96];
    if (log_n < 1 || log_n > 24 || !deep_plan_check(limits, m, group_columns, group_pairs, n_groups, n_points, pair_point, why)) return -1;
    DeepRoundsLaunch launches[DEEP_R_GROUPS];
    const u32 count = deep_rounds_split(group_columns, group_pairs, n_groups, pair_point, launches);
    DeepGroupsArgs common{};
    common.limb_stride = limb_stride; common.n = 1ull << log_n; common.offset = offset;
    std::vector<u64> omegas;
    deep_host_omega_tables(common, omega, log_n, omegas);
    const Xfe lam = xfe_load3(lambda);
    Xfe scale{{1, 0, 0}};
    for (u32 l = 0; l < count; ++l) {
        DeepGroupsArgs a = common;
        deep_rounds_args(a, launches[l], columns, is_ext, group_columns, group_pairs, points, pair_point, pair_values, lam, scale);
        deep_with_count<DEEP_G_POINTS>(launches[l].n_points, [&](auto np) {
            if (l == 0) launch_np<decltype(np)::value, false>(a, out, out_stride);
            else launch_np<decltype(np)::value, true>(a, out, out_stride);
            return 0;
        });
    }
    return (int)count;
}

}  // namespace

extern "C" unsigned emu_deep_rounds_limits(unsigned* out) {
    out[0] = DEEP_R_LIMITS.columns; out[1] = DEEP_R_LIMITS.groups; out[2] = DEEP_R_LIMITS.points; out[3] = DEEP_R_LIMITS.pairs;
    out[4] = DEEP_G_LIMITS.columns; out[5] = DEEP_G_LIMITS.groups; out[6] = DEEP_G_LIMITS.points; out[7] = DEEP_G_LIMITS.pairs;
    return 8;
}

// deep_rounds_split; out: 16 words per launch -- first_group, n_groups, first_column, n_columns, first_pair, n_pairs, n_points, 0, and
// the plan's indices of its points.  -> the number of launches, -1: a plan the rounds entry refuses
extern "C" int emu_deep_rounds_split(unsigned m, const unsigned* group_columns, const unsigned* group_pairs, unsigned n_groups, unsigned n_points,
                                     const unsigned* pair_point, unsigned* out) {
    char why[96];
    if (!deep_plan_check(DEEP_R_LIMITS, m, group_columns, group_pairs, n_groups, n_points, pair_point, why)) return -1;
    DeepRoundsLaunch launches[DEEP_R_GROUPS];
    const u32 count = deep_rounds_split(group_columns, group_pairs, n_groups, pair_point, launches);
    for (u32 l = 0; l < count; ++l) {
        const DeepRoundsLaunch& L = launches[l];
        const u32 head[8] = {L.first_group, L.n_groups, L.first_column, L.n_columns, L.first_pair, L.n_pairs, L.n_points, 0};
        for (u32 w = 0; w < 8; ++w) out[16 * l + w] = head[w];
        for (u32 p = 0; p < DEEP_G_POINTS; ++p) out[16 * l + 8 + p] = p < L.n_points ? L.point[p] : 0xFFFFFFFFu;
    }
    return (int)count;
}

// bfsx_deep_quotient_groups as its launch computes it.  columns[c]: the codeword's first word, IN GROUP ORDER; is_ext[c].
// -> 0, -1: arguments the entry point refuses
extern "C" int emu_deep_quotient_groups(const u64* const* columns, const int* is_ext, unsigned m, u64 limb_stride, unsigned log_n, u64 offset, u64 omega,
                                        const unsigned* group_columns, const unsigned* group_pairs, unsigned n_groups, const u64* points,
                                        unsigned n_points, const unsigned* pair_point, const u64* pair_values, const u64* lambda, u64* out, u64 out_stride) {
    return plan_quotient(DEEP_G_LIMITS, columns, is_ext, m, limb_stride, log_n, offset, omega, group_columns, group_pairs, n_groups, points, n_points,
                         pair_point, pair_values, lambda, out, out_stride) == 1 ? 0 : -1;
}

// bfsr_deep_quotient_rounds as its launches compute it; the arguments are emu_deep_quotient_groups'.
// -> the number of launches, -1: arguments the entry point refuses
extern "C" int emu_deep_quotient_rounds(const u64* const* columns, const int* is_ext, unsigned m, u64 limb_stride, unsigned log_n, u64 offset, u64 omega,
                                        const unsigned* group_columns, const unsigned* group_pairs, unsigned n_groups, const u64* points,
                                        unsigned n_points, const unsigned* pair_point, const u64* pair_values, const u64* lambda, u64* out, u64 out_stride) {
    return plan_quotient(DEEP_R_LIMITS, columns, is_ext, m, limb_stride, log_n, offset, omega, group_columns, group_pairs, n_groups, points, n_points,
                         pair_point, pair_values, lambda, out, out_stride);
}
