/*
 * bfstark_compose.h -- the entry points of libbfstark_hip.so for the COMPOSITION polynomial of a proof by out-of-domain openings
 * (stark_brainfuck_amd/brainfuck_stark.py: BrainfuckStark.prove_deep; DESIGN.md, "Proving by out-of-domain openings"):
 *
 *     H(x) = sum over tables t, quotients q of  beta_{t,q} * quotient_{t,q}(x)  +  sum over j < 2 of  beta_j * (lhs_j - rhs_j)(x) / (x - 1)
 *
 * evaluated straight from the trace codewords, on every 2^log_step-th point of the domain x_i = offset * omega^i, i < N = 2^log_n.  The
 * quotients are bfs_air_quotients' (constraint value times the inverse of the kind's zerofier: 1 / (x - 1) boundary,
 * (x - omicron^-1) / (x^height - 1) transition -- 0 for height 0 --, 1 / (x - omicron^-1) terminal) and are never written.  Against
 * bfs_air_combine there are no column terms, no second weight per term and no powers of x: H has degree < N / expansion_factor as it
 * stands, which is also why a caller needs it on every expansion_factor-th point only.
 *
 * Why a header of its own, and a fourth prefix.  tests/test_gpu_pcs.py pins the library's exported bfs_* symbols beyond bfstark.h to the
 * two of bfstark_ext.h (bfsx_ and bfsr_ are pinned by their own tests), and the change that added these entries left existing test files
 * and headers as they were.  So the entries carry the prefix bfsc_, are declared here, bound through _lib._COMPOSE_SIGNATURES (loaded
 * together with the other tables), and tests/test_gpu_deep_stark.py carries for them the stream-order legs and the comparison of exports,
 * header and signature table.
 *
 * Conventions are bfstark.h's: BFS_ERR_* codes and bfs_last_error(), canonical residues mod p = 2^64 - 2^32 + 1, codewords column-major
 * (base column c at d_base[c * N + i], extension column c as three limb planes at d_ext[(3 c + limb) * N + i]), d_* device and h_* host
 * pointers, `stream` a hipStream_t as void*.  Both entries ONLY ENQUEUE one kernel: they neither synchronise nor copy nor allocate; what
 * they read from h_* pointers has been read when they return (weights, challenges, terminals and parameters travel by value).
 *
 * d_acc: three limb planes of N >> log_step words each, one behind the other; entry k belongs to domain point k << log_step.
 * accumulate == 0: the entries are written and never read (d_acc needs no initialisation); accumulate != 0: the sum is added to them.
 * Nothing beyond the 3 * (N >> log_step) words is touched.  d_acc may not overlap a codeword.
 */
#ifndef BFSTARK_COMPOSE_H
#define BFSTARK_COMPOSE_H

#include "bfstark.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * bfsc_air_compose   d_acc[k] (+)= sum_q beta_q * quotient_{table,q}(x_{k << log_step}),  q < bfs_air_num_quotients(table) in boundary,
 *     transition, terminal order, beta_q = h_weights[3 q .. 3 q + 3).  table, d_base, d_ext, log_n, unit_distance, height, omicron_inv,
 *     offset, omega, h_challenges (11 x 3), h_terminals (5 x 3) and h_params (1 x 3, or null for a table without a parameter) are
 *     bfs_air_quotients' arguments; the row after point i is read at (i + unit_distance) mod N of the full codewords, whatever log_step.
 *     BFS_ERR_BAD_ARG: table outside 0..4, log_n > 32, log_step > log_n, a null d_base, d_ext, d_acc, h_challenges, h_terminals or
 *     h_weights; BFS_ERR_NOT_POW2: a height that is neither zero nor a power of two; BFS_ERR_NOT_ROOT as bfs_air_quotients.  A refused
 *     call enqueues nothing.
 */
int bfsc_air_compose(int table, const uint64_t* d_base, const uint64_t* d_ext, uint32_t log_n, uint64_t unit_distance, uint64_t height,
                     uint64_t omicron_inv, uint64_t offset, uint64_t omega, const uint64_t* h_challenges, const uint64_t* h_terminals,
                     const uint64_t* h_params, const uint64_t* h_weights, uint32_t log_step, int accumulate, uint64_t* d_acc, void* stream);

/*
 * bfsc_difference_compose   d_acc[k] (+)= beta * (lhs(x_i) - rhs(x_i)) / (x_i - 1),  i = k << log_step, for two extension codewords of
 *     three limb planes N words apart (the running products of a permutation argument) and beta = h_weight[0..3).
 *     BFS_ERR_BAD_ARG: log_n > 32, log_step > log_n, a null pointer; BFS_ERR_NOT_ROOT as above.  A refused call enqueues nothing.
 */
int bfsc_difference_compose(const uint64_t* d_lhs, const uint64_t* d_rhs, uint32_t log_n, uint64_t offset, uint64_t omega,
                            const uint64_t* h_weight, uint32_t log_step, int accumulate, uint64_t* d_acc, void* stream);

#ifdef __cplusplus
}
#endif

#endif
