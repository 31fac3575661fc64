// segments.hip -- the commitment codewords of a proof by out-of-domain openings on a trace-sized domain (include/bfstark_segments.h;
// BrainfuckStark.prove_deep(segmented=True)): every 2^log_step-th word of each codeword on the working domain, gathered into a dense
// buffer in pcs.Commitment's layout.  One thread per output word, one grid row per codeword: the loads of a wavefront touch 2^log_step
// times as many cache lines as its stores, which is all the kernel costs (profiles/deep_stark_segmented.md has the figures).
#include <cstdint>

#include "../../include/bfstark_segments.h"
#include "runtime.hpp"

namespace bfs {

__global__ __launch_bounds__(256) void decimate_rows_kernel(const uint64_t* __restrict__ in, uint64_t stride_in, uint32_t log_step,
                                                            uint64_t* __restrict__ out, uint64_t stride_out, uint64_t n_out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t row = blockIdx.y;
    if (i < n_out) out[row * stride_out + i] = in[row * stride_in + (i << log_step)];
}

}  // namespace bfs

using namespace bfs;

extern "C" {

int bfsg_decimate_rows(const uint64_t* d_in, uint64_t stride_in, uint32_t log_step, uint64_t* d_out, uint64_t stride_out, uint64_t n_out,
                       uint32_t batch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!d_in || !d_out) { set_error("bfsg_decimate_rows: null pointer"); return BFS_ERR_BAD_ARG; }
    if (log_step > 32) { set_error("bfsg_decimate_rows: need log_step <= 32 (got %u)", log_step); return BFS_ERR_BAD_ARG; }
    // (i << log_step with i < 2^32 and log_step <= 32 stays below 2^64; the grid's x extent stays below 2^24 blocks)
    if (n_out == 0 || n_out > (1ull << 32)) { set_error("bfsg_decimate_rows: need 1 <= n_out <= 2^32 (got %llu)", (unsigned long long)n_out); return BFS_ERR_BAD_ARG; }
    if (stride_out < n_out) { set_error("bfsg_decimate_rows: output rows overlap (stride_out < n_out)"); return BFS_ERR_BAD_ARG; }
    if (batch > 65535) { set_error("bfsg_decimate_rows: at most 65535 rows (got %u)", batch); return BFS_ERR_BAD_ARG; }
    if (batch == 0) return BFS_OK;
    hipLaunchKernelGGL(decimate_rows_kernel, dim3((uint32_t)((n_out + 255) / 256), batch), dim3(256), 0, stream, d_in, stride_in, log_step, d_out,
                       stride_out, n_out);
    BFS_HIP(hipGetLastError());
    return BFS_OK;
}

}  // extern "C"
