/*
 * bfstark_rounds.h -- the entry point of libbfstark_hip.so for opening the polynomials of SEVERAL commitments under one opening plan
 * and one low-degree test (stark_brainfuck_amd/pcs.py: PolynomialCommitment.open_rounds / verify_rounds).  An interactive oracle proof
 * commits in rounds -- later columns depend on challenges drawn from earlier roots -- and opens everything at once at the end; the
 * quotient of such an opening has up to 96 columns, which is more than one launch of bfsx_deep_quotient_groups takes.
 *
 * Why a header of its own, and a third prefix.  tests/test_gpu_pcs.py pins the library's exported bfs_* symbols beyond bfstark.h to
 * the two of bfstark_ext.h, and tests/test_gpu_pcs_groups.py pins the exported bfsx_* symbols to exactly the two of bfstark_open.h.
 * The change that added this entry left existing test files and the three headers as they were, so the entry carries the prefix
 * bfsr_, which neither pattern matches, is declared here, bound through _lib._ROUNDS_SIGNATURES (loaded together with the other three
 * tables), and tests/test_gpu_pcs_rounds.py carries for it the stream-order leg and the comparison of exports, header and signature
 * table.  Folding the headers into one is a later change.
 *
 * Conventions are bfstark_open.h's.  The entry ONLY ENQUEUES: it neither synchronises nor copies nor allocates; what it reads from
 * h_* pointers has been read when it returns.
 */
#ifndef BFSTARK_ROUNDS_H
#define BFSTARK_ROUNDS_H

#include "bfstark_open.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * bfsr_deep_quotient_rounds   bfsx_deep_quotient_groups' quotient, argument for argument, of a plan with wider limits: 1 <= m <= 96
 *     codewords IN GROUP ORDER (they may lie in the buffers of different commitments; limb_stride is the one distance between the planes
 *     of every extension codeword), 1 <= n_groups <= 24, 1 <= n_points <= 24 distinct points, at most 48 pairs, 1 <= h_group_pairs[g] <= 4,
 *     1 <= h_group_columns[g] <= 32 and their sum = m.  base(q), S_g, Y_q and g[i] are bfsx_deep_quotient_groups' over the WHOLE plan.
 *     The sum over the groups is split between launches by one rule: groups in plan order; a launch takes groups while its columns <= 32,
 *     its groups <= 8, its pairs <= 16 and the distinct points among its groups <= 8; the first group that would break one of these
 *     starts the next launch.  The first launch writes d_out and never reads it (d_out needs no initialisation); every later launch
 *     starts each g[i] from what d_out holds.  Field addition is exact, so the split changes no word of the result.  A plan that fits
 *     one launch is enqueued as bfsx_deep_quotient_groups enqueues it.  All launches go to `stream` in order.
 *     h_launches: when not null, receives the number of launches.
 *     BFS_ERR_BAD_ARG: what bfsx_deep_quotient_groups refuses, against the limits above, and a group of more than 32 columns;
 *     BFS_ERR_NOT_ROOT when omega is not a primitive N-th root of unity.  A refused call enqueues nothing.
 */
int bfsr_deep_quotient_rounds(const bfs_row_column* h_columns, uint32_t m, uint64_t limb_stride, uint32_t log_n, uint64_t offset, uint64_t omega,
                              const uint32_t* h_group_columns, const uint32_t* h_group_pairs, uint32_t n_groups, const uint64_t* h_points,
                              uint32_t n_points, const uint32_t* h_pair_point, const uint64_t* h_pair_values, const uint64_t h_lambda[3],
                              uint64_t* d_out, uint64_t out_stride, uint32_t* h_launches, void* stream);

#ifdef __cplusplus
}
#endif

#endif
