/*
 * bfstark_open.h -- entry points of libbfstark_hip.so for opening each committed polynomial at its own set of points
 * (stark_brainfuck_amd/pcs.py: PolynomialCommitment.open_at / verify_at).  They extend the two of bfstark_ext.h: evaluation of SEPARATE
 * coefficient columns in one call, and the DEEP quotient of an opening plan -- groups of columns, each with its own points.
 *
 * Why a header of its own, and another prefix.  tests/test_gpu_pcs.py asserts that the library's exported bfs_* symbols beyond
 * bfstark.h are exactly the two of bfstark_ext.h, and tests/test_host_logic.py that bfstark.h and _lib._SIGNATURES list the same
 * names.  The change that added these entries left existing test files, bfstark.h and bfstark_ext.h as they were, so the entries
 * carry the prefix bfsx_, which neither test's pattern matches, are declared here, bound through _lib._OPEN_SIGNATURES (loaded together
 * with the other two tables), and tests/test_gpu_pcs_groups.py carries for them the stream-order legs and the comparison of exports,
 * header and signature table.  Folding the three headers into one is a later change.
 *
 * Conventions are bfstark_ext.h's: BFS_ERR_* codes and bfs_last_error(), canonical residues mod p = 2^64 - 2^32 + 1, limb-major extension
 * arrays, d_* device and h_* host pointers, `stream` a hipStream_t as void*.  Both entries ONLY ENQUEUE: they neither synchronise nor
 * copy; what they read from h_* pointers has been read when they return (it travels with the launches as kernel arguments).
 */
#ifndef BFSTARK_OPEN_H
#define BFSTARK_OPEN_H

#include "bfstark_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bfsx_eval_column {
    const uint64_t* d_coeffs; /* BASE-field coefficients, lowest first */
    uint64_t n_coeffs;        /* 1 .. 2^24 */
} bfsx_eval_column;

/*
 * bfsx_poly_eval_columns   d_out[(b * k + j) * 3 + l] = limb l of  f_b(z_j) = sum_{i < n_b} c_b[i] * z_j^i,  as bfs_poly_eval_points writes
 *     it, for `count` columns that are separate arrays of their own lengths: c_b = h_columns[b].d_coeffs, n_b = h_columns[b].n_coeffs.
 *     1 <= count <= 96, 1 <= n_b <= 2^24, 1 <= k <= 4.  Three launches whatever count is: the table of the points, the per-workgroup
 *     partial sums over a grid (workgroups of the longest column, count) -- a workgroup past the end of its own column contributes
 *     nothing -- and one launch that combines, per column, as many partial sums as that column has.  d_out: 3 * count * k words that
 *     overlap no column.  BFS_ERR_BAD_ARG: a count or a length out of range, a null column, a point that is not reduced, an overlap.
 */
int bfsx_poly_eval_columns(const bfsx_eval_column* h_columns, uint32_t count, const uint64_t* h_points, uint32_t k, uint64_t* d_out, void* stream);

/*
 * bfsx_deep_quotient_groups   the DEEP quotient of an opening plan over x_i = offset * omega^i, i < N = 2^log_n.  The m codewords are given
 *     IN GROUP ORDER: group g < n_groups owns the next h_group_columns[g] of them, f_{g,0} .. , and the next h_group_pairs[g] of the
 *     (group, point) pairs; pair q opens its group at the point z = h_points[3 h_pair_point[q] ..) of the n_points distinct points.  With
 *     base(q) = the number of columns of all pairs in front of q (pair q counts its group's columns) and lambda = h_lambda[0..3):
 *         g[i] = sum_g sum_{q of g} ( lambda^base(q) * S_g(x_i) - Y_q ) / (x_i - z_q),    S_g(x) = sum_r lambda^r * f_{g,r}(x),
 *     where Y_q = h_pair_values[3 q ..) is the caller's  sum_r lambda^(base(q) + r) * y_{q,r}  for the claimed values y_{q,r} = f_{g,r}(z_q).
 *     One group of all columns is bfs_deep_quotient's formula word for word.  One launch: per point of the domain the inverses
 *     1 / (x_i - z) are taken once per DISTINCT point (they share one base-field inversion), every codeword is read once and enters
 *     exactly one sum S_g.  Codewords, strides and d_out are bfs_deep_quotient's; no point may lie in the domain (the caller checks).
 *     1 <= m <= 32, 1 <= n_groups <= 8, 1 <= n_points <= 8, at most 16 pairs, 1 <= h_group_pairs[g] <= 4, 1 <= h_group_columns[g] and
 *     their sum = m, 1 <= log_n <= 24, limb_stride >= N, out_stride >= N.  BFS_ERR_BAD_ARG: any of these violated, h_pair_point[q] >=
 *     n_points, one point twice in a group, unreduced words, d_out overlapping a codeword; BFS_ERR_NOT_ROOT when omega is not a primitive
 *     N-th root of unity.
 */
int bfsx_deep_quotient_groups(const bfs_row_column* h_columns, uint32_t m, uint64_t limb_stride, uint32_t log_n, uint64_t offset, uint64_t omega,
                              const uint32_t* h_group_columns, const uint32_t* h_group_pairs, uint32_t n_groups, const uint64_t* h_points,
                              uint32_t n_points, const uint32_t* h_pair_point, const uint64_t* h_pair_values, const uint64_t h_lambda[3],
                              uint64_t* d_out, uint64_t out_stride, void* stream);

#ifdef __cplusplus
}
#endif

#endif
