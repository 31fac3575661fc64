/*
 * bfstark_segments.h -- the entry point of libbfstark_hip.so that a proof by out-of-domain openings on a TRACE-SIZED commitment domain
 * needs beyond bfstark_compose.h (stark_brainfuck_amd/brainfuck_stark.py: BrainfuckStark.prove_deep(segmented=True); DESIGN.md,
 * "Segmented composition"):
 *
 * the trace columns are extended once onto a working domain of W = 2^k N' points (the composition polynomial needs them there), and the
 * commitments are made on the N' points offset * omega_W^(i W / N'), i.e. on every (W / N')-th word of every codeword.  The entry below
 * gathers those words of all codewords of a commitment into a dense buffer in pcs.Commitment's layout, in one launch.
 *
 * Why a header of its own, and a fifth prefix.  tests/test_gpu_deep_stark.py pins the bfsc_ exports to the two of bfstark_compose.h, and
 * other tests pin bfs_, bfsx_ and bfsr_; the change that added this entry left existing test files and headers as they were.  So the
 * entry carries the prefix bfsg_, is declared here, bound through _lib._SEGMENTS_SIGNATURES (loaded together with the other tables), and
 * tests/test_gpu_deep_segmented.py carries for it the stream-order leg and the comparison of exports, header and signature table.
 *
 * Conventions are bfstark.h's: BFS_ERR_* codes and bfs_last_error(), d_* device pointers, `stream` a hipStream_t as void*.  The entry
 * ONLY ENQUEUES one kernel: it neither synchronises nor copies nor allocates.
 */
#ifndef BFSTARK_SEGMENTS_H
#define BFSTARK_SEGMENTS_H

#include "bfstark.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * bfsg_decimate_rows   d_out[r * stride_out + i] = d_in[r * stride_in + (i << log_step)]   for r < batch, i < n_out  (64-bit words).
 *     Rows of the input lie stride_in words apart and must hold ((n_out - 1) << log_step) + 1 words; rows of the output lie stride_out
 *     words apart, stride_out >= n_out.  Nothing beyond the n_out words of each of the batch output rows is written, the input is only
 *     read; the two may not overlap.  batch == 0 enqueues nothing and is no error.
 *     BFS_ERR_BAD_ARG: a null d_in or d_out, log_step > 32, n_out == 0 or n_out > 2^32, stride_out < n_out, batch > 65535.  A refused
 *     call enqueues nothing.
 */
int bfsg_decimate_rows(const uint64_t* d_in, uint64_t stride_in, uint32_t log_step, uint64_t* d_out, uint64_t stride_out, uint64_t n_out,
                       uint32_t batch, void* stream);

#ifdef __cplusplus
}
#endif

#endif
