// blind.hip -- the two blinding kernels of the zero-knowledge mode of prove_deep (include/bfstark_blind.h; BrainfuckStark.prove_deep(
// zero_knowledge=True); DESIGN.md, "Zero-knowledge openings"): f + (X^h - 1) r on the rows of a coefficient buffer, in place, and the
// blinded segments of the composition polynomial.  Both are elementwise and bandwidth-bound, in the mould of decimate_rows_kernel
// (segments.hip): one thread per output word (8 bytes per lane, coalesced), one grid row per polynomial or limb plane, no LDS, no scratch.
// The per-word bodies are csrc/blind_core.hpp's, which tests/emu/emu_blind.cpp compiles for the host.
#include <cstdint>

#include "../../include/bfstark_blind.h"
#include "blind_core.hpp"
#include "runtime.hpp"

namespace bfs {

__global__ __launch_bounds__(256) void poly_blind_kernel(uint64_t* __restrict__ coeffs, uint64_t stride, uint64_t h, const uint64_t* __restrict__ blind,
                                                         uint64_t blind_stride, uint64_t k) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t row = blockIdx.y;
    if (i < h + k) coeffs[row * stride + i] = poly_blind_word(coeffs[row * stride + i], blind + row * blind_stride, i, h, k);
}

__global__ __launch_bounds__(256) void split_blind_kernel(const uint64_t* __restrict__ hp, uint64_t h_stride, uint64_t S, uint64_t L0, uint32_t s,
                                                          const uint64_t* __restrict__ b, uint64_t b_stride, uint64_t m, uint64_t* __restrict__ out,
                                                          uint64_t out_stride) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t j = blockIdx.y / 3, l = blockIdx.y % 3;
    if (c < L0 + m) out[(uint64_t)blockIdx.y * out_stride + c] = split_blind_word(hp, h_stride, S, L0, s, b, b_stride, m, j, l, c);
}

}  // namespace bfs

using namespace bfs;

extern "C" {

int bfsz_poly_blind(uint64_t* d_coeffs, uint64_t stride, uint64_t h, uint32_t batch, const uint64_t* d_blind, uint64_t blind_stride, uint64_t k,
                    void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!d_coeffs || !d_blind) { set_error("bfsz_poly_blind: null pointer"); return BFS_ERR_BAD_ARG; }
    // (h, k <= 2^32: h + k cannot wrap, and the grid's x extent stays below 2^25 blocks)
    if (k == 0 || k > (1ull << 32)) { set_error("bfsz_poly_blind: need 1 <= k <= 2^32 (got %llu)", (unsigned long long)k); return BFS_ERR_BAD_ARG; }
    if (h == 0 || h > (1ull << 32)) { set_error("bfsz_poly_blind: need 1 <= h <= 2^32 (got %llu)", (unsigned long long)h); return BFS_ERR_BAD_ARG; }
    if (stride < h + k) { set_error("bfsz_poly_blind: a row does not hold h + k coefficients (stride < h + k)"); return BFS_ERR_BAD_ARG; }
    if (blind_stride < k) { set_error("bfsz_poly_blind: blinding rows overlap (blind_stride < k)"); return BFS_ERR_BAD_ARG; }
    if (batch == 0 || batch > 65535) { set_error("bfsz_poly_blind: 1 .. 65535 rows (got %u)", batch); return BFS_ERR_BAD_ARG; }
    hipLaunchKernelGGL(poly_blind_kernel, dim3((uint32_t)((h + k + 255) / 256), batch), dim3(256), 0, stream, d_coeffs, stride, h, d_blind, blind_stride, k);
    BFS_HIP(hipGetLastError());
    return BFS_OK;
}

int bfsz_split_blind(const uint64_t* d_h, uint64_t h_stride, uint64_t S, uint64_t L0, uint32_t s, const uint64_t* d_b, uint64_t b_stride, uint64_t m,
                     uint64_t* d_out, uint64_t out_stride, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!d_h || !d_out || (!d_b && m != 0)) { set_error("bfsz_split_blind: null pointer"); return BFS_ERR_BAD_ARG; }
    if (L0 == 0 || L0 > (1ull << 32)) { set_error("bfsz_split_blind: need 1 <= L0 <= 2^32 (got %llu)", (unsigned long long)L0); return BFS_ERR_BAD_ARG; }
    if (m > L0) { set_error("bfsz_split_blind: need m <= L0 (got %llu > %llu)", (unsigned long long)m, (unsigned long long)L0); return BFS_ERR_BAD_ARG; }
    if (s == 0 || s > 16) { set_error("bfsz_split_blind: 1 .. 16 segments (got %u)", s); return BFS_ERR_BAD_ARG; }
    if (S == 0 || (uint64_t)s * L0 < S) { set_error("bfsz_split_blind: the segments do not cover the polynomial (need 1 <= S <= s * L0)"); return BFS_ERR_BAD_ARG; }
    if (h_stride < S) { set_error("bfsz_split_blind: limb planes overlap (h_stride < S)"); return BFS_ERR_BAD_ARG; }
    if (m != 0 && b_stride < m) { set_error("bfsz_split_blind: blinding planes overlap (b_stride < m)"); return BFS_ERR_BAD_ARG; }
    if (out_stride < L0 + m) { set_error("bfsz_split_blind: output planes overlap (out_stride < L0 + m)"); return BFS_ERR_BAD_ARG; }
    hipLaunchKernelGGL(split_blind_kernel, dim3((uint32_t)((L0 + m + 255) / 256), 3 * s), dim3(256), 0, stream, d_h, h_stride, S, L0, s, d_b, b_stride, m,
                       d_out, out_stride);
    BFS_HIP(hipGetLastError());
    return BFS_OK;
}

}  // extern "C"
