// Host emulation of the launches behind include/bfstark_rounds.h (csrc/deep.hip over csrc/deep_core.hpp): the quotient of a plan over
// the columns of several commitments.  The split between launches is the library's own function (deep_rounds_split), the arguments of
// every launch the library's own (deep_rounds_args), and every thread of every workgroup of every launch runs the kernel's per-thread
// code -- the first launch from zero without reading the output, every later one from what the output holds.  TEST INFRASTRUCTURE, see
// emu_ntt.cpp.
#include <vector>

#include "../../stark_brainfuck_amd/csrc/deep_core.hpp"

using namespace bfs;

namespace {

template <int NP, bool ACC>
void rounds_np(const DeepGroupsArgs& a, u64* out, u64 out_stride) {
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

template <bool ACC>
void rounds_launch(u32 n_points, const DeepGroupsArgs& a, u64* out, u64 out_stride) {
    switch (n_points) {
    case 1: rounds_np<1, ACC>(a, out, out_stride); break;
    case 2: rounds_np<2, ACC>(a, out, out_stride); break;
    case 3: rounds_np<3, ACC>(a, out, out_stride); break;
    case 4: rounds_np<4, ACC>(a, out, out_stride); break;
    case 5: rounds_np<5, ACC>(a, out, out_stride); break;
    case 6: rounds_np<6, ACC>(a, out, out_stride); break;
    case 7: rounds_np<7, ACC>(a, out, out_stride); break;
    default: rounds_np<8, ACC>(a, out, out_stride); break;
    }
}

bool plan_is_taken(unsigned m, const unsigned* group_columns, const unsigned* group_pairs, unsigned n_groups, unsigned n_points, const unsigned* pair_point) {
    if (m < 1 || m > DEEP_R_COLUMNS || n_groups < 1 || n_groups > DEEP_R_GROUPS || n_points < 1 || n_points > DEEP_R_POINTS) return false;
    u32 columns = 0, pairs = 0;
    for (u32 g = 0; g < n_groups; ++g) {
        if (group_columns[g] < 1 || group_columns[g] > DEEP_MAX_COLUMNS || columns + group_columns[g] > m) return false;
        if (group_pairs[g] < 1 || group_pairs[g] > DEEP_MAX_POINTS || pairs + group_pairs[g] > DEEP_R_PAIRS) return false;
        for (u32 j = 0; j < group_pairs[g]; ++j)
            if (pair_point[pairs + j] >= n_points) return false;
        columns += group_columns[g]; pairs += group_pairs[g];
    }
    return columns == m;
}

}  // namespace

extern "C" unsigned emu_deep_rounds_limits(unsigned* out) {
    out[0] = DEEP_R_COLUMNS; out[1] = DEEP_R_GROUPS; out[2] = DEEP_R_POINTS; out[3] = DEEP_R_PAIRS;
    out[4] = DEEP_MAX_COLUMNS; out[5] = DEEP_G_GROUPS; out[6] = DEEP_G_POINTS; out[7] = DEEP_G_PAIRS;
    return 8;
}

// deep_rounds_split; out: 16 words per launch -- first_group, n_groups, first_column, n_columns, first_pair, n_pairs, n_points, 0, and
// the plan's indices of its points.  -> the number of launches, -1: a plan the entry point refuses
extern "C" int emu_deep_rounds_split(unsigned m, const unsigned* group_columns, const unsigned* group_pairs, unsigned n_groups, unsigned n_points,
                                     const unsigned* pair_point, unsigned* out) {
    if (!plan_is_taken(m, group_columns, group_pairs, n_groups, n_points, pair_point)) return -1;
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

// bfsr_deep_quotient_rounds as its launches compute it.  columns[c]: the codeword's first word, IN GROUP ORDER; is_ext[c].
// -> the number of launches, -1: arguments the entry point refuses
extern "C" int emu_deep_quotient_rounds(const u64* const* columns, const int* is_ext, unsigned m, u64 limb_stride, unsigned log_n, u64 offset, u64 omega,
                                        const unsigned* group_columns, const unsigned* group_pairs, unsigned n_groups, const u64* points,
                                        unsigned n_points, const unsigned* pair_point, const u64* pair_values, const u64* lambda, u64* out, u64 out_stride) {
    if (log_n < 1 || log_n > 24 || !plan_is_taken(m, group_columns, group_pairs, n_groups, n_points, pair_point)) return -1;
    DeepRoundsLaunch launches[DEEP_R_GROUPS];
    const u32 count = deep_rounds_split(group_columns, group_pairs, n_groups, pair_point, launches);
    DeepGroupsArgs common{};
    common.limb_stride = limb_stride; common.n = 1ull << log_n; common.offset = offset;
    common.lo_bits = (log_n + 1) / 2;                     // the two-level table of the launch
    std::vector<u64> lo(1ull << common.lo_bits), hi(1ull << (log_n - common.lo_bits));
    for (u64 i = 0; i < lo.size(); ++i) lo[i] = gl_pow(omega, i);
    for (u64 i = 0; i < hi.size(); ++i) hi[i] = gl_pow(omega, i << common.lo_bits);
    common.w_lo = lo.data(); common.w_hi = hi.data();
    const Xfe lam = xfe_load3(lambda);
    Xfe scale{{1, 0, 0}};
    for (u32 l = 0; l < count; ++l) {
        DeepGroupsArgs a = common;
        deep_rounds_args(a, launches[l], columns, is_ext, group_columns, group_pairs, points, pair_point, pair_values, lam, scale);
        if (l == 0) rounds_launch<false>(launches[l].n_points, a, out, out_stride);
        else rounds_launch<true>(launches[l].n_points, a, out, out_stride);
    }
    return (int)count;
}
