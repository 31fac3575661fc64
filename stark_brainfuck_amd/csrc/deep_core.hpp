// deep_core.hpp -- the per-thread half of the two kernels of deep.hip, host/device, so that tests/emu/emu_deep.cpp runs it against
// CPython integers:
//   1. out-of-domain evaluation  f(z_j) = sum_i c_i z_j^i  of a column of BASE coefficients at up to four points of F_p^3;
//   2. the DEEP quotient  g[i] = sum_j (lambda^(j m) S_i - Y_j) / (x_i - z_j),  S_i = sum_p lambda^p f_p(x_i),  over x_i = offset omega^i.
//
// Evaluation.  A workgroup of T = 256 threads owns B = T * S = 16384 consecutive coefficients; thread t takes c[b B + s T + t], s < S
// (coalesced), and
//     sum_{s, t} c[b B + s T + t] z^(s T + t) = sum_t z^t * ( sum_s c[..] * (z^T)^s ).
// The inner sum has the SAME weight (z^T)^s in every lane -- a table of S elements per point -- so a coefficient costs one
// base-by-extension product per point, three base products, accumulated without reduction (lazy.hpp: 24 VALU instructions); the
// thread's sum is reduced once and multiplied by the lane's own z^t (the only extension-by-extension product, one per S coefficients),
// the workgroup adds its 256 values, and the combining launch scales workgroup b's sum by (z^B)^b.  Horner's rule would pay nine base
// products and a reduction per coefficient and could not share a load between the points.
//
// Quotient.  A thread owns E = 2 points of the domain.  S_i is one unreduced weighted sum over the m codewords (lazy.hpp, the weights
// lambda^p wave-uniform), whatever k is.  1 / (x - z) for x in F_p is adj / norm with the cofactors and the norm of the matrix of
// multiplication by (x - z0) - z1 X - z2 X^2 (pointwise.hip: xfe_cofactors_kernel); z1 and z2 do not depend on the point of the domain,
// so their products are constants of the launch.  The E * k norms of a thread share ONE base-field inversion (Montgomery's trick).
//
// The two entries of include/bfstark_open.h reuse both: evaluation of separate columns of different lengths in one launch, and the
// quotient of an opening plan (groups of columns, each with its own points); their parts of this file say what is new.  The entry of
// include/bfstark_rounds.h splits a plan over the columns of several commitments between launches of that kernel (the last part).
//
// The host side of a plan is here ONCE, for both plan entries of deep.hip and for their emulations under tests/emu: deep_plan_check
// (is the plan within the entry's limits), deep_rounds_split (which groups go into which launch) and deep_rounds_args (the only
// function that fills a DeepGroupsArgs).  deep_with_count turns a run-time number of points into a template argument for all of them.
#pragma once
#include <stddef.h>
#include <stdio.h>

#include <type_traits>
#include <vector>

#include "lazy.hpp"

namespace bfs {

constexpr u32 DEEP_MAX_POINTS = 4;
constexpr u32 DEEP_MAX_COLUMNS = 32;                       // bfs_merkle_build_rows' limit
constexpr u32 DEEP_EVAL_T = 256;                           // threads of a workgroup = distance between two coefficients of a thread
constexpr u32 DEEP_EVAL_S = 64;                            // coefficients of a thread
constexpr u32 DEEP_EVAL_BLOCK = DEEP_EVAL_T * DEEP_EVAL_S; // coefficients of a workgroup
// the table of one launch, words: lane factors z_j^t at ((j T + t) * 3), behind all of them the step weights z_j^(T s) at ((j S + s) * 3)
constexpr u32 DEEP_EVAL_STEPS_AT = DEEP_MAX_POINTS * DEEP_EVAL_T * 3;
constexpr u32 DEEP_EVAL_TABLE_WORDS = DEEP_EVAL_STEPS_AT + DEEP_MAX_POINTS * DEEP_EVAL_S * 3;

struct DeepPoints {
    Xfe z[DEEP_MAX_POINTS];
};

BFS_HD Xfe xfe_load3(const u64* w) { return Xfe{{w[0], w[1], w[2]}}; }

BFS_HD Xfe xfe_pow_small(Xfe a, u64 e) {
    Xfe acc{{1, 0, 0}};
    while (e) {
        if (e & 1) acc = xfe_mul(acc, a);
        e >>= 1;
        if (e) a = xfe_mul(a, a);
    }
    return acc;
}

// fn(std::integral_constant<int, count>()) for 1 <= count <= MAX (the caller has checked the range): a run-time number of points as a
// template argument.  Only 1 .. MAX are instantiated
template <int MAX, class Fn>
inline int deep_with_count(u32 count, Fn&& fn) {
    if constexpr (MAX > 1) {
        if (count < (u32)MAX) return deep_with_count<MAX - 1>(count, fn);
    }
    return fn(std::integral_constant<int, MAX>());
}

// the two-level powers of omega that the quotient kernels index (runtime.hpp: ntt_power_tables), in host memory for the emulations:
// a.w_lo[i] = omega^i, a.w_hi[i] = omega^(i << a.lo_bits); `words` owns them.  A: DeepQuotientArgs or DeepGroupsArgs
template <class A>
inline void deep_host_omega_tables(A& a, u64 omega, u32 log_n, std::vector<u64>& words) {
    a.lo_bits = (log_n + 1) / 2;
    const u64 lo = 1ull << a.lo_bits, hi = 1ull << (log_n - a.lo_bits);
    words.resize(lo + hi);
    for (u64 i = 0; i < lo; ++i) words[i] = gl_pow(omega, i);
    for (u64 i = 0; i < hi; ++i) words[lo + i] = gl_pow(omega, i << a.lo_bits);
    a.w_lo = words.data(); a.w_hi = words.data() + lo;
}

// entry t < T of point j's part of the table (and, for t < S, step weight t)
BFS_HD void deep_eval_table_entry(const Xfe& z, u32 j, u32 t, u64* table) {
    const Xfe lane = xfe_pow_small(z, t);
    u64* at = table + ((size_t)j * DEEP_EVAL_T + t) * 3;
    at[0] = lane.c[0]; at[1] = lane.c[1]; at[2] = lane.c[2];
    if (t < DEEP_EVAL_S) {
        const Xfe step = xfe_pow_small(z, (u64)t * DEEP_EVAL_T);
        u64* st = table + DEEP_EVAL_STEPS_AT + ((size_t)j * DEEP_EVAL_S + t) * 3;
        st[0] = step.c[0]; st[1] = step.c[1]; st[2] = step.c[2];
    }
}

// thread t of workgroup `block`: z_j^t * sum_s col[block B + s T + t] * z_j^(T s), j < K.  steps: K * S * 3 words, point-major (LDS on
// the device); lanes: the table's lane factors
template <int K>
BFS_HD void deep_eval_thread(const u64* col, u64 n, u64 block, u32 t, const u64* steps, const u64* lanes, Xfe out[K]) {
    LazyX acc[K];
    BFS_UNROLL
    for (int j = 0; j < K; ++j) acc[j] = lazyx_zero();
    const u64 first = block * DEEP_EVAL_BLOCK + t;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4
#endif
    for (u32 s = 0; s < DEEP_EVAL_S; ++s) {
        const u64 i = first + (u64)s * DEEP_EVAL_T;
        const u64 c = i < n ? col[i] : 0;
        BFS_UNROLL
        for (int j = 0; j < K; ++j) lazyx_mac_base(acc[j], steps + ((size_t)j * DEEP_EVAL_S + s) * 3, c);
    }
    BFS_UNROLL
    for (int j = 0; j < K; ++j) out[j] = xfe_mul(lazyx_reduce(acc[j]), xfe_load3(lanes + ((size_t)j * DEEP_EVAL_T + t) * 3));
}

// z^B from the table of point j: z^(T (S - 1)) * z^T
BFS_HD Xfe deep_eval_block_power(const u64* table, u32 j) {
    const u64* st = table + DEEP_EVAL_STEPS_AT + (size_t)j * DEEP_EVAL_S * 3;
    return xfe_mul(xfe_load3(st + (DEEP_EVAL_S - 1) * 3), xfe_load3(st + 3));
}

// ---- evaluation of separate columns in one call (include/bfstark_open.h: bfsx_poly_eval_columns) ----
// The same launches over a grid (blocks of the LONGEST column, columns): pointers and lengths are kernel arguments, a workgroup past
// the end of its own column leaves, and the combining launch adds only the deep_eval_blocks(n_b) partial sums that column b has.
constexpr u32 DEEP_EVAL_MAX_COLUMNS = 96;

struct DeepEvalColumns {
    const u64* col[DEEP_EVAL_MAX_COLUMNS];
    u32 n[DEEP_EVAL_MAX_COLUMNS];                          // 1 .. 2^24 coefficients
};

BFS_HD u32 deep_eval_blocks(u64 n) { return (u32)((n + DEEP_EVAL_BLOCK - 1) / DEEP_EVAL_BLOCK); }
// word at which workgroup `block` of column b leaves its sum for point j of k; row_blocks: the blocks of the longest column
BFS_HD size_t deep_eval_partial_at(u32 b, u32 k, u32 j, u32 row_blocks, u32 block) { return (((size_t)b * k + j) * row_blocks + block) * 3; }

// ---- the quotient ----
constexpr u32 DEEP_Q_T = 256;      // threads of a workgroup
constexpr u32 DEEP_Q_E = 2;         // points of a thread, DEEP_Q_T apart

struct DeepPointConsts {            // of one z = (z0, z1, z2), with a1 = -z1, a2 = -z2, d = a1 - a2
    u64 z0, a1, a2, d_a1, d_a2, a1_sq;
    Xfe scale;                      // lambda^(j m)
    Xfe y;                          // Y_j
};

struct DeepQuotientArgs {
    const u64* col[DEEP_MAX_COLUMNS];
    u64 weight[DEEP_MAX_COLUMNS][LAZY_W_EXT];      // lambda^p as lazy.hpp lays a weight out (a base column reads the first three words)
    DeepPointConsts pt[DEEP_MAX_POINTS];
    u32 m, ext_mask;                // bit p: column p is an extension column (three planes, limb_stride apart)
    u64 limb_stride, n, offset;
    const u64* w_lo;                // two-level powers of omega
    const u64* w_hi;
    u32 lo_bits;
};

inline void deep_point_consts(DeepPointConsts& c, const Xfe& z, const Xfe& scale, const Xfe& y) {
    c.z0 = z.c[0];
    c.a1 = gl_neg(z.c[1]);
    c.a2 = gl_neg(z.c[2]);
    const u64 d = gl_sub(c.a1, c.a2);
    c.d_a1 = gl_mul(d, c.a1);
    c.d_a2 = gl_mul(d, c.a2);
    c.a1_sq = gl_mul(c.a1, c.a1);
    c.scale = scale;
    c.y = y;
}

// the weighted sum of the codewords first .. last - 1 at point i (A: DeepQuotientArgs or DeepGroupsArgs)
template <class A>
BFS_HD Xfe deep_range_sum(const A& a, u32 first, u32 last, u64 i) {
    LazyX L = lazyx_zero();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
    for (u32 p = first; p < last; ++p) {
        const u64* w = a.weight[p];
        const u64* src = a.col[p];
        if ((a.ext_mask >> p) & 1) {
            const Xfe v{{src[i], src[a.limb_stride + i], src[2 * a.limb_stride + i]}};
            lazy_mac(L.r[0], v.c[0], w[0]); lazy_mac(L.r[0], v.c[1], w[3]); lazy_mac(L.r[0], v.c[2], w[4]);
            lazy_mac(L.r[1], v.c[0], w[1]); lazy_mac(L.r[1], v.c[1], w[5]); lazy_mac(L.r[1], v.c[2], w[6]);
            lazy_mac(L.r[2], v.c[0], w[2]); lazy_mac(L.r[2], v.c[1], w[1]); lazy_mac(L.r[2], v.c[2], w[5]);
        } else {
            const u64 v = src[i];
            lazy_mac(L.r[0], v, w[0]); lazy_mac(L.r[1], v, w[1]); lazy_mac(L.r[2], v, w[2]);
        }
    }
    return lazyx_reduce(L);
}

// S_i: the weighted sum of the m codewords at point i
BFS_HD Xfe deep_row_sum(const DeepQuotientArgs& a, u64 i) { return deep_range_sum(a, 0, a.m, i); }

// cofactors and norm of the matrix of multiplication by x - z (x in F_p): 1 / (x - z) = cof / norm
BFS_HD u64 deep_cofactors(const u64 x, u64 z0, u64 a1, u64 a2, u64 d_a1, u64 d_a2, u64 a1_sq, Xfe& cof) {
    const u64 a0 = gl_sub(x, z0);
    const u64 s = gl_add(a0, a2);
    const u64 c0 = gl_sub(gl_mul(s, s), d_a1);                       // (a0+a2)^2 - (a1-a2) a1
    const u64 c1 = gl_sub(d_a2, gl_mul(a1, s));                      // (a1-a2) a2 - a1 (a0+a2)
    const u64 c2 = gl_sub(a1_sq, gl_mul(s, a2));                     // a1^2 - (a0+a2) a2
    const u64 nm = gl_sub(gl_mul(a0, c0), gl_add(gl_mul(a2, c1), gl_mul(a1, c2)));
    cof = Xfe{{c0, c1, c2}};
    return nm == 0 ? 1 : nm;      // x = z: the caller has refused such points; the thread's other inverses stay right
}

// the E points idx[e] of one thread (idx[e] >= n: none); K points z_j
template <int K>
BFS_HD void deep_quotient_thread(const DeepQuotientArgs& a, const u64 idx[DEEP_Q_E], Xfe out[DEEP_Q_E]) {
    Xfe sum[DEEP_Q_E], cof[DEEP_Q_E][K];
    u64 norm[DEEP_Q_E][K], before[DEEP_Q_E][K];
    u64 run = 1;
    BFS_UNROLL
    for (u32 e = 0; e < DEEP_Q_E; ++e) {
        const bool live = idx[e] < a.n;
        const u64 i = live ? idx[e] : 0;
        sum[e] = deep_row_sum(a, i);
        const u64 x = gl_mul(a.offset, gl_mul(a.w_lo[i & ((1ull << a.lo_bits) - 1)], a.w_hi[i >> a.lo_bits]));
        BFS_UNROLL
        for (int j = 0; j < K; ++j) {
            const DeepPointConsts& c = a.pt[j];
            const u64 nm = deep_cofactors(x, c.z0, c.a1, c.a2, c.d_a1, c.d_a2, c.a1_sq, cof[e][j]);
            norm[e][j] = nm;
            before[e][j] = run;
            run = gl_mul(run, nm);
        }
    }
    u64 inv = gl_inv(run);
    BFS_UNROLL
    for (int e = DEEP_Q_E - 1; e >= 0; --e) {
        LazyX G = lazyx_zero();
        BFS_UNROLL
        for (int j = K - 1; j >= 0; --j) {
            const u64 ninv = gl_mul(inv, before[e][j]);
            inv = gl_mul(inv, norm[e][j]);
            const Xfe scaled = j == 0 ? sum[e] : xfe_mul(sum[e], a.pt[j].scale);      // (lambda^0 = 1)
            const Xfe num = xfe_sub(scaled, a.pt[j].y);
            lazyx_mac_scale(G, xfe_mul(num, cof[e][j]), ninv);
        }
        out[e] = lazyx_reduce(G);
    }
}

// ---- the quotient of an opening plan (include/bfstark_open.h: bfsx_deep_quotient_groups) ----
// The columns lie in group order; group g owns the columns col_end[g-1] .. col_end[g] - 1 and the pairs pair_end[g-1] .. pair_end[g] - 1,
// a pair being (lambda^base, Y, index of its point among the distinct points).  A thread first takes 1 / (x - z) for every DISTINCT
// point (one shared inversion, as above), then goes group by group: S_g, and per pair of the group (scale * S_g - Y) / (x - z).
// Nothing is indexed by a run-time value in registers: the pair's point is picked by a chain of wave-uniform selects.
constexpr u32 DEEP_G_GROUPS = 8;
constexpr u32 DEEP_G_POINTS = 8;    // distinct points of a plan
constexpr u32 DEEP_G_PAIRS = 16;    // (group, point) pairs of a plan
constexpr u32 DEEP_G_T = 256;       // threads of a workgroup
// points of the domain per thread, DEEP_G_T apart: the (cofactors, norm, running product) sets a thread holds are E * distinct points
constexpr u32 deep_groups_e(u32 n_points) { return n_points <= DEEP_MAX_POINTS ? 2 : 1; }

struct DeepGroupPoint {             // DeepPointConsts without the pair's part
    u64 z0, a1, a2, d_a1, d_a2, a1_sq;
};

struct DeepGroupPair {
    Xfe scale;                      // lambda^base[g][j]
    Xfe y;                          // Y_{g,j}
    u32 point;                      // < n_points
    u32 unit;                       // scale = 1: no product
};

struct DeepGroupsArgs {
    const u64* col[DEEP_MAX_COLUMNS];
    u64 weight[DEEP_MAX_COLUMNS][LAZY_W_EXT];      // lambda^r, r = the column's place in its group
    DeepGroupPoint pt[DEEP_G_POINTS];
    DeepGroupPair pair[DEEP_G_PAIRS];
    u32 col_end[DEEP_G_GROUPS], pair_end[DEEP_G_GROUPS];
    u32 n_groups, ext_mask;
    u64 limb_stride, n, offset;
    const u64* w_lo;
    const u64* w_hi;
    u32 lo_bits;
};

inline void deep_group_point(DeepGroupPoint& c, const Xfe& z) {
    DeepPointConsts full;
    deep_point_consts(full, z, Xfe{{1, 0, 0}}, Xfe{{0, 0, 0}});
    c.z0 = full.z0; c.a1 = full.a1; c.a2 = full.a2; c.d_a1 = full.d_a1; c.d_a2 = full.d_a2; c.a1_sq = full.a1_sq;
}

// the E points idx[e] of one thread (idx[e] >= n: none); NP distinct points; the sum over the pairs starts from start[e] (an earlier
// launch's share of the same opening, see "openings across commitments" below)
template <int NP, int E>
BFS_HD void deep_groups_thread_from(const DeepGroupsArgs& a, const u64 idx[E], const Xfe start[E], Xfe out[E]) {
    Xfe cof[E][NP];
    u64 norm[E][NP], before[E][NP], at[E];
    u64 run = 1;
    BFS_UNROLL
    for (int e = 0; e < E; ++e) {
        at[e] = idx[e] < a.n ? idx[e] : 0;
        const u64 x = gl_mul(a.offset, gl_mul(a.w_lo[at[e] & ((1ull << a.lo_bits) - 1)], a.w_hi[at[e] >> a.lo_bits]));
        BFS_UNROLL
        for (int p = 0; p < NP; ++p) {
            const DeepGroupPoint& c = a.pt[p];
            norm[e][p] = deep_cofactors(x, c.z0, c.a1, c.a2, c.d_a1, c.d_a2, c.a1_sq, cof[e][p]);
            before[e][p] = run;
            run = gl_mul(run, norm[e][p]);
        }
    }
    u64 inv = gl_inv(run);
    BFS_UNROLL
    for (int e = E - 1; e >= 0; --e) {
        BFS_UNROLL
        for (int p = NP - 1; p >= 0; --p) {
            const u64 ninv = gl_mul(inv, before[e][p]);
            inv = gl_mul(inv, norm[e][p]);
            norm[e][p] = ninv;                                     // from here on: 1 / norm
        }
    }
    Xfe g[E];
    BFS_UNROLL
    for (int e = 0; e < E; ++e) g[e] = start[e];
    u32 c0 = 0, q0 = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
    for (u32 grp = 0; grp < a.n_groups; ++grp) {
        const u32 c1 = a.col_end[grp], q1 = a.pair_end[grp];
        Xfe sum[E];
        BFS_UNROLL
        for (int e = 0; e < E; ++e) sum[e] = deep_range_sum(a, c0, c1, at[e]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
        for (u32 q = q0; q < q1; ++q) {
            const DeepGroupPair& pr = a.pair[q];
            BFS_UNROLL
            for (int e = 0; e < E; ++e) {
                Xfe c = cof[e][0];
                u64 ninv = norm[e][0];
                BFS_UNROLL
                for (int p = 1; p < NP; ++p) {
                    const bool here = pr.point == (u32)p;
                    c.c[0] = here ? cof[e][p].c[0] : c.c[0]; c.c[1] = here ? cof[e][p].c[1] : c.c[1]; c.c[2] = here ? cof[e][p].c[2] : c.c[2];
                    ninv = here ? norm[e][p] : ninv;
                }
                const Xfe num = xfe_sub(pr.unit ? sum[e] : xfe_mul(sum[e], pr.scale), pr.y);
                const Xfe term = xfe_mul(num, c);
                g[e] = xfe_add(g[e], Xfe{{gl_mul(term.c[0], ninv), gl_mul(term.c[1], ninv), gl_mul(term.c[2], ninv)}});
            }
        }
        c0 = c1; q0 = q1;
    }
    BFS_UNROLL
    for (int e = 0; e < E; ++e) out[e] = g[e];
}

// a whole plan in one launch: the sum starts from zero
template <int NP, int E>
BFS_HD void deep_groups_thread(const DeepGroupsArgs& a, const u64 idx[E], Xfe out[E]) {
    Xfe zero[E];
    BFS_UNROLL
    for (int e = 0; e < E; ++e) zero[e] = Xfe{{0, 0, 0}};
    deep_groups_thread_from<NP, E>(a, idx, zero, out);
}

// ---- openings across commitments (include/bfstark_rounds.h: bfsr_deep_quotient_rounds) ----
// A plan over the columns of several commitments is larger than one launch takes: up to 96 columns, 24 groups, 24 distinct points,
// 48 pairs.  The sum over the groups is split between launches -- field addition is exact, so the split changes no word of g: the first
// launch writes g, every later one starts from what it finds there (deep_groups_thread_from).  The pairs carry lambda^base as `scale`,
// so a later launch simply receives its pairs' powers; a launch gets only the distinct points its own groups use, re-indexed in order of
// first appearance, and with them its own NP and E.  The rule is the one function below, which tests/emu/emu_deep_rounds.cpp runs too.
constexpr u32 DEEP_R_COLUMNS = 96;
constexpr u32 DEEP_R_GROUPS = 24;
constexpr u32 DEEP_R_POINTS = 24;
constexpr u32 DEEP_R_PAIRS = 48;

struct DeepPlanLimits {
    u32 columns, groups, points, pairs;
};
constexpr DeepPlanLimits DEEP_G_LIMITS{DEEP_MAX_COLUMNS, DEEP_G_GROUPS, DEEP_G_POINTS, DEEP_G_PAIRS};      // bfsx_deep_quotient_groups: one launch
constexpr DeepPlanLimits DEEP_R_LIMITS{DEEP_R_COLUMNS, DEEP_R_GROUPS, DEEP_R_POINTS, DEEP_R_PAIRS};        // bfsr_deep_quotient_rounds

// THE check of a plan as the entries receive it (host only): within `lim`, every group with 1..32 columns and 1..4 pairs, the sizes
// adding up to m, every pair naming one of the n_points points and no point twice in a group.  false: `why` says what is wrong
inline bool deep_plan_check(const DeepPlanLimits& lim, u32 m, const u32* group_columns, const u32* group_pairs, u32 n_groups, u32 n_points,
                            const u32* pair_point, char (&why)[96]) {
    const auto refuse = [&](const char* what, u32 a, u32 b) { snprintf(why, sizeof why, what, a, b); return false; };
    if (m < 1 || m > lim.columns) return refuse("1..%u codewords (got %u)", lim.columns, m);
    if (n_groups < 1 || n_groups > lim.groups) return refuse("1..%u groups (got %u)", lim.groups, n_groups);
    if (n_points < 1 || n_points > lim.points) return refuse("1..%u distinct points (got %u)", lim.points, n_points);
    u32 columns = 0, pairs = 0;
    for (u32 g = 0; g < n_groups; ++g) {
        if (group_columns[g] < 1 || group_columns[g] > m - columns) return refuse("group %u: an empty group, or more columns than there are (%u)", g, m);
        if (group_columns[g] > DEEP_MAX_COLUMNS) return refuse("group %u: at most 32 columns in a group (got %u)", g, group_columns[g]);
        if (group_pairs[g] < 1 || group_pairs[g] > DEEP_MAX_POINTS) return refuse("group %u: 1..4 points (got %u)", g, group_pairs[g]);
        if (group_pairs[g] > lim.pairs - pairs) return refuse("at most %u (group, point) pairs (group %u goes beyond)", lim.pairs, g);
        u32 seen = 0;
        for (u32 j = 0; j < group_pairs[g]; ++j) {
            const u32 point = pair_point[pairs + j];
            if (point >= n_points) return refuse("pair %u names point %u, which is none of the plan's", pairs + j, point);
            if ((seen >> point) & 1) return refuse("group %u opens point %u twice", g, point);
            seen |= 1u << point;
        }
        columns += group_columns[g];
        pairs += group_pairs[g];
    }
    if (columns != m) return refuse("the groups hold %u columns, not %u", columns, m);
    return true;
}

struct DeepRoundsLaunch {
    u32 first_group, n_groups;
    u32 first_column, n_columns;
    u32 first_pair, n_pairs;
    u32 n_points;
    u32 point[DEEP_G_POINTS];       // the plan's index of the launch's point p < n_points
};

// Groups in plan order; a launch takes groups while its columns <= 32, its groups <= 8, its pairs <= 16 and the distinct points among
// its groups <= 8; the first group that would break one of these starts the next launch.  Every group has 1..32 columns and 1..4 pairs
// (deep_plan_check), so a group alone always fits.  Every bound here is one of the one-launch limits (DEEP_G_LIMITS), so a plan within
// those is always exactly ONE launch.  launches: room for n_groups entries.  -> the number of launches
inline u32 deep_rounds_split(const u32* group_columns, const u32* group_pairs, u32 n_groups, const u32* pair_point, DeepRoundsLaunch* launches) {
    u32 count = 0, c = 0, q = 0;
    DeepRoundsLaunch cur{};
    for (u32 g = 0; g < n_groups; ++g) {
        for (int attempt = 0; attempt < 2; ++attempt) {
            u32 pts[DEEP_G_POINTS + DEEP_MAX_POINTS], np = cur.n_points;
            for (u32 p = 0; p < np; ++p) pts[p] = cur.point[p];
            for (u32 j = 0; j < group_pairs[g]; ++j) {
                u32 p = 0;
                while (p < np && pts[p] != pair_point[q + j]) ++p;
                if (p == np) pts[np++] = pair_point[q + j];
            }
            if (cur.n_columns + group_columns[g] <= DEEP_MAX_COLUMNS && cur.n_groups + 1 <= DEEP_G_GROUPS && cur.n_pairs + group_pairs[g] <= DEEP_G_PAIRS &&
                np <= DEEP_G_POINTS) {
                cur.n_groups += 1; cur.n_columns += group_columns[g]; cur.n_pairs += group_pairs[g]; cur.n_points = np;
                for (u32 p = 0; p < np; ++p) cur.point[p] = pts[p];
                break;
            }
            launches[count++] = cur;                       // (never on the second attempt: a group alone fits)
            cur = DeepRoundsLaunch{};
            cur.first_group = g; cur.first_column = c; cur.first_pair = q;
        }
        c += group_columns[g]; q += group_pairs[g];
    }
    launches[count++] = cur;
    return count;
}

// the plan's part of launch L's arguments (the caller fills n, strides, offset and the tables of omega).  col / is_ext: the columns of
// the WHOLE plan in group order; points, pair_point, pair_values: the whole plan's.  scale: lambda^base of L's first pair on entry, of
// the next launch's first pair on return.  The launch's points are those its pairs name, in order of first appearance (L.point): a
// point of the plan that no pair uses reaches no kernel, and the kernel's NP is the number of points in use.
inline void deep_rounds_args(DeepGroupsArgs& a, const DeepRoundsLaunch& L, const u64* const* col, const int* is_ext, const u32* group_columns,
                             const u32* group_pairs, const u64* points, const u32* pair_point, const u64* pair_values, const Xfe& lambda, Xfe& scale) {
    a.n_groups = L.n_groups;
    a.ext_mask = 0;
    for (u32 p = 0; p < L.n_points; ++p) deep_group_point(a.pt[p], xfe_load3(points + 3 * (size_t)L.point[p]));
    u32 c = 0, q = 0;
    for (u32 g = 0; g < L.n_groups; ++g) {
        Xfe power{{1, 0, 0}};                             // lambda^r
        for (u32 r = 0; r < group_columns[L.first_group + g]; ++r, ++c) {
            a.col[c] = col[L.first_column + c];
            if (is_ext[L.first_column + c]) a.ext_mask |= 1u << c;
            lazy_weight_matrix(power, a.weight[c]);
            power = xfe_mul(power, lambda);
        }
        for (u32 j = 0; j < group_pairs[L.first_group + g]; ++j, ++q) {
            DeepGroupPair& pr = a.pair[q];
            u32 p = 0;
            while (L.point[p] != pair_point[L.first_pair + q]) ++p;          // (deep_rounds_split put it there)
            pr.scale = scale; pr.y = xfe_load3(pair_values + 3 * (size_t)(L.first_pair + q)); pr.point = p;
            pr.unit = scale.c[0] == 1 && scale.c[1] == 0 && scale.c[2] == 0;
            scale = xfe_mul(scale, power);                // power = lambda^|columns_g| here
        }
        a.col_end[g] = c; a.pair_end[g] = q;
    }
}

}  // namespace bfs
