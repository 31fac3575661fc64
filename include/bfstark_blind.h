/*
 * bfstark_blind.h -- the two entry points of libbfstark_hip.so that the ZERO-KNOWLEDGE mode of a proof by out-of-domain openings needs
 * beyond bfstark_compose.h and bfstark_segments.h (stark_brainfuck_amd/deep_stark.py; BrainfuckStark.prove_deep(zero_knowledge=True);
 * DESIGN.md, "Zero-knowledge openings"):
 *
 *   bfsz_poly_blind    f' = f + (X^h - 1) r on every row of a coefficient buffer: the trace interpolants keep their values on the trace
 *                      subgroup (X^h = 1 there) and take k blinding coefficients;
 *   bfsz_split_blind   the composition polynomial H cut into s pieces of L0 coefficients, piece j blinded as
 *                      H_j' = H_j + X^L0 b_j - b_{j-1}, so that sum_j X^(j L0) H_j' = H still holds exactly.
 *
 * Why a seventh header, and a sixth prefix (bfs_ of bfstark.h and bfstark_ext.h, bfsx_, bfsr_, bfsc_, bfsg_ came before): existing tests pin
 * the exports of the six earlier headers to fixed sets (bfstark_segments.h says how that came about).  The entries carry the prefix bfsz_,
 * are declared here, bound through _lib._BLIND_SIGNATURES (loaded together with the other tables), and tests/test_gpu_blind_kernels.py
 * compares exports, header and signature table.
 *
 * Conventions are bfstark.h's: BFS_ERR_* codes and bfs_last_error(), d_* device pointers, `stream` a hipStream_t as void*, words are
 * 64-bit.  Each entry ONLY ENQUEUES one kernel on `stream`: it neither synchronises nor copies nor allocates, and writes nothing outside
 * the words named below.  A refused call enqueues nothing.
 */
#ifndef BFSTARK_BLIND_H
#define BFSTARK_BLIND_H

#include "bfstark.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * bfsz_poly_blind   for every row b < batch (rows of d_coeffs lie `stride` words apart, rows r_b of d_blind `blind_stride` words) and
 *     every i < h + k, in place:
 *         new[i] = old[i] - (i < k ? r_b[i] : 0) + (i >= h ? r_b[i - h] : 0)   mod p.
 *     Each word is computed from the old word at its own position, so k > h is as good as k <= h.  The old coefficients are canonical
 *     residues (what the transforms write; the caller has zeroed the words behind the interpolant); the blinding words may be any 64-bit
 *     values and are reduced.  The result is canonical.  Nothing beyond the h + k words of each of the batch rows is written; d_blind is
 *     only read; the two may not overlap.
 *     BFS_ERR_BAD_ARG: a null d_coeffs or d_blind; k == 0; h == 0; h or k above 2^32; stride < h + k; blind_stride < k; batch == 0 or
 *     batch > 65535.
 */
int bfsz_poly_blind(uint64_t* d_coeffs, uint64_t stride, uint64_t h, uint32_t batch, const uint64_t* d_blind, uint64_t blind_stride, uint64_t k,
                    void* stream);

/*
 * bfsz_split_blind   d_h: three limb planes of S coefficients, h_stride words apart.  d_b: the blinding polynomials b_0 .. b_{s-2}, three
 *     limb planes of m words each, plane l of b_j at d_b + (3 j + l) * b_stride.  d_out: s segments of three planes of L0 + m words in
 *     pcs.Commitment's layout, plane l of segment j at d_out + (3 j + l) * out_stride:
 *         out[j][l][c] = (c < L0 and j L0 + c < S ? H[l][j L0 + c] : 0) + (c >= L0 and j < s - 1 ? b[j][l][c - L0] : 0)
 *                        - (c < m and j >= 1 ? b[j - 1][l][c] : 0)   mod p     for c < L0 + m.
 *     All input words may be any 64-bit values and are reduced; the result is canonical.  Nothing beyond the L0 + m words of each of the
 *     3 s output planes is written; the inputs are only read and may not overlap the output.  With m == 0 (no blinding: the plain
 *     segments) d_b is not looked at and may be null.
 *     BFS_ERR_BAD_ARG: a null d_h or d_out, a null d_b with m > 0; m > L0; L0 == 0 or above 2^32; s == 0 or s > 16; S == 0 or
 *     s * L0 < S; h_stride < S; b_stride < m; out_stride < L0 + m.
 */
int bfsz_split_blind(const uint64_t* d_h, uint64_t h_stride, uint64_t S, uint64_t L0, uint32_t s, const uint64_t* d_b, uint64_t b_stride, uint64_t m,
                     uint64_t* d_out, uint64_t out_stride, void* stream);

#ifdef __cplusplus
}
#endif

#endif
