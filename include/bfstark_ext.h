/*
 * bfstark_ext.h -- entry points of libbfstark_hip.so that came after bfstark.h: opening committed polynomials at points outside
 * the FRI domain (stark_brainfuck_amd/pcs.py: PolynomialCommitment, evaluate_at).  The reference has no counterpart: its STARK never
 * evaluates a committed polynomial off the domain, so each entry names the formula it computes instead of a reference call.
 *
 * Why a header of its own.  Two tests are pinned to bfstark.h: tests/test_stream_cases_host.py wants a case in tests/stream_cases.py
 * for every stream-taking function it declares, and tests/test_host_logic.py wants it and _lib._SIGNATURES to list the same names.
 * The change that added these entries left existing test files as they were, so the entries are declared here, bound through
 * _lib._EXT_SIGNATURES (loaded together with _SIGNATURES), and tests/test_gpu_pcs.py carries for them what those two tests carry
 * for bfstark.h: the stream-order legs and the comparison of exports, header and signature table.  Folding the two headers together
 * is a later change.
 *
 * Conventions are bfstark.h's: BFS_ERR_* codes and bfs_last_error(), canonical residues mod p = 2^64 - 2^32 + 1, limb-major extension
 * arrays, d_* device and h_* host pointers, `stream` a hipStream_t as void*.  Both entries ONLY ENQUEUE: they neither synchronise nor
 * copy; what they read from h_* pointers has been read when they return.
 */
#ifndef BFSTARK_EXT_H
#define BFSTARK_EXT_H

#include "bfstark.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * bfs_poly_eval_points   d_out[(b * k + j) * 3 + l] = limb l of  f_b(z_j) = sum_{i < n_coeffs} c_b[i] * z_j^i  in F_p[X]/(X^3 - X + 1),
 *     c_b = the n_coeffs BASE-field coefficients at d_coeffs + b * in_stride (b < batch), z_j = h_points[3 j .. 3 j + 3), j < k.
 *     An extension polynomial is three such columns (its limb planes); its value is v0 + X v1 + X^2 v2 of the columns' values.
 *     1 <= n_coeffs <= 2^24 (any number), 1 <= batch <= 65535, 1 <= k <= 4.  One pass over the coefficients serves all k points: a
 *     launch of per-workgroup partial sums and one that combines them (csrc/deep.hip), no atomics.  d_out: 3 * batch * k words that
 *     do not overlap the coefficients.  BFS_ERR_BAD_ARG: a count out of range, in_stride < n_coeffs, a point that is not reduced.
 */
int bfs_poly_eval_points(const uint64_t* d_coeffs, uint64_t n_coeffs, uint64_t in_stride, uint32_t batch, const uint64_t* h_points,
                         uint32_t k, uint64_t* d_out, void* stream);

/*
 * bfs_deep_quotient   the DEEP quotient of m committed codewords f_0 .. f_{m-1} over x_i = offset * omega^i, i < N = 2^log_n, at the
 *     k points z_j = h_points[3 j ..), with the challenge lambda = h_lambda[0..3):
 *         g[i] = sum_{j < k} ( lambda^(j m) * S_i - Y_j ) / (x_i - z_j),    S_i = sum_{p < m} lambda^p * f_p(x_i),
 *     where Y_j = h_values[3 j ..) is the caller's  sum_{p < m} lambda^(j m + p) * y_{p,j}  for the claimed values y_{p,j} = f_p(z_j).
 *     g is the codeword of a polynomial of degree < max deg f_p exactly when every claim is true.  Codewords are described as for
 *     bfs_merkle_build_rows (field_id is not looked at): a base column is N words, an extension column three planes limb_stride
 *     words apart.  Every codeword is read once whatever k is; the k inverses per point share base-field inversions.
 *     d_out: limb planes out_stride words apart; it may not overlap a codeword.  No z_j may lie in the domain: the caller checks
 *     (PolynomialCommitment.open refuses such points); the kernel has no flag, and a point that does gives a meaningless g[i] there.
 *     1 <= m <= 32, 1 <= k <= 4, 1 <= log_n <= 24, limb_stride >= N, out_stride >= N.  Errors: BFS_ERR_BAD_ARG; BFS_ERR_NOT_ROOT when
 *     omega is not a primitive N-th root of unity.
 */
int bfs_deep_quotient(const bfs_row_column* h_columns, uint32_t m, uint64_t limb_stride, uint32_t log_n, uint64_t offset, uint64_t omega,
                      const uint64_t* h_points, const uint64_t* h_values, uint32_t k, const uint64_t h_lambda[3], uint64_t* d_out,
                      uint64_t out_stride, void* stream);

#ifdef __cplusplus
}
#endif

#endif
