// pointwise.hip -- element-wise kernels over the base field and its cubic extension: pointwise product, batch inverse, scale
// the four-instruction subtraction, as in ntt.hip (gl.hpp: gl_sub4)
#define BFS_GL_SUB4
#include "runtime.hpp"

namespace bfs {

// ---- element-wise kernels (ntt.py:76, ntt.py:177-188, univariate.py:168-169) ----
__global__ void gl_mul_pointwise_kernel(const u64* a, const u64* b, u64* out, u64 n) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) out[i] = gl_mul(a[i], b[i]);
}

// batch_inverse (ntt.py:177-188) by Montgomery's trick at workgroup scope: 2048 elements share ONE field inversion.
// Thread t holds elements base + k * 256 + t (k < 8, coalesced), multiplies them up, the 256 thread products are scanned from
// both ends in LDS (Kogge-Stone, 8 steps each), thread 0 inverts the workgroup's product (the only a^(p-2): 64 squarings), and
// every thread unwinds: 1 / (its product) = 1 / total * (product of the threads before) * (product of the threads after), then
// element by element.  ~5 multiplications per element instead of ~96.  Zeros (the reference asserts there are none, ntt.py:180
// "batch inverse does not work when input contains a zero") are taken out of the products, reported through `zero_flag` and
// get inverse(0) = 0 (algebra.py:101-103) in the output.
constexpr int BINV_T = 256, BINV_E = 8;
__global__ void __launch_bounds__(BINV_T) gl_batch_inverse_kernel(const u64* in, u64* out, u64 n, unsigned int* zero_flag) {
    __shared__ u64 pre[BINV_T], suf[BINV_T];
    __shared__ u64 inv_total;
    const u32 tid = threadIdx.x;
    const u64 base = (u64)blockIdx.x * (BINV_T * BINV_E);
    u64 v[BINV_E], before[BINV_E];
    bool zero[BINV_E];
    u64 prod = 1;
    bool any_zero = false;
    BFS_UNROLL
    for (int k = 0; k < BINV_E; ++k) {
        const u64 i = base + (u64)k * BINV_T + tid;
        const u64 x = i < n ? in[i] : 1;
        zero[k] = x == 0;
        any_zero |= zero[k];
        v[k] = zero[k] ? 1 : x;
        before[k] = prod;                        // product of this thread's elements 0..k-1
        prod = gl_mul(prod, v[k]);
    }
    if (any_zero) *(volatile unsigned int*)zero_flag = 1u;    // pinned host memory; every writer stores the same value
    pre[tid] = prod;
    suf[tid] = prod;
    __syncthreads();
    // inclusive scans: pre[t] = prod of threads 0..t, suf[t] = prod of threads t..255
    for (u32 d = 1; d < BINV_T; d <<= 1) {
        const u64 a = tid >= d ? pre[tid - d] : 1, b = tid + d < BINV_T ? suf[tid + d] : 1;
        const u64 p0 = pre[tid], s0 = suf[tid];
        __syncthreads();
        pre[tid] = gl_mul(p0, a);
        suf[tid] = gl_mul(s0, b);
        __syncthreads();
    }
    if (tid == 0) inv_total = gl_inv(pre[BINV_T - 1]);
    __syncthreads();
    u64 run = inv_total;                         // -> 1 / (product of this thread's elements)
    if (tid > 0) run = gl_mul(run, pre[tid - 1]);
    if (tid + 1 < BINV_T) run = gl_mul(run, suf[tid + 1]);
    BFS_UNROLL
    for (int k = BINV_E - 1; k >= 0; --k) {
        const u64 i = base + (u64)k * BINV_T + tid;
        const u64 r = gl_mul(run, before[k]);    // 1 / v[k]
        if (i < n) out[i] = zero[k] ? 0 : r;
        run = gl_mul(run, v[k]);
    }
}

// ---- the same two over the cubic extension (limb planes): the Hadamard product of fast_multiply (ntt.py:76) and the batch_inverse of
// fast_coset_divide (ntt.py:226) when Table.ldex interpolates extension columns (table.py:133-134 -> ntt.py:126-161 -> 82-98 -> 45-79)
__global__ void xfe_mul_pointwise_kernel(const u64* a, u64 a_stride, const u64* b, u64 b_stride, u64* out, u64 out_stride, u64 n) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const Xfe x{{a[i], a[a_stride + i], a[2 * a_stride + i]}}, y{{b[i], b[b_stride + i], b[2 * b_stride + i]}};
        const Xfe r = xfe_mul(x, y);
        out[i] = r.c[0]; out[out_stride + i] = r.c[1]; out[2 * out_stride + i] = r.c[2];
    }
}

// 1 / a = adj(M_a) e_0 / det(M_a), M_a the matrix of multiplication by a = a0 + a1 X + a2 X^2 modulo X^3 - X + 1:
//     M_a = [ a0  -a2      -a1     ]
//           [ a1   a0+a2    a1-a2  ]
//           [ a2   a1       a0+a2  ]
// det(M_a) is the norm of a, an element of F_p that is zero only for a = 0: the norms go through the base field's batch inversion
// (one field inversion per 2048 elements) and the cofactors are scaled by the result.
__global__ void xfe_cofactors_kernel(const u64* in, u64 in_stride, u64* out, u64 out_stride, u64* norm, u64 n) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 a0 = in[i], a1 = in[in_stride + i], a2 = in[2 * in_stride + i];
        const u64 s = gl_add(a0, a2), d = gl_sub(a1, a2);
        const u64 c0 = gl_sub(gl_mul(s, s), gl_mul(d, a1));                      // (a0+a2)^2 - (a1-a2) a1
        const u64 c1 = gl_sub(gl_mul(d, a2), gl_mul(a1, s));                      // (a1-a2) a2 - a1 (a0+a2)
        const u64 c2 = gl_sub(gl_mul(a1, a1), gl_mul(s, a2));                     // a1^2 - (a0+a2) a2
        norm[i] = gl_sub(gl_mul(a0, c0), gl_add(gl_mul(a2, c1), gl_mul(a1, c2))); // first row of M_a times the cofactors
        out[i] = c0; out[out_stride + i] = c1; out[2 * out_stride + i] = c2;
    }
}

__global__ void xfe_scale_by_kernel(u64* x, u64 stride, const u64* f, u64 n) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 s = f[i];
        x[i] = gl_mul(x[i], s); x[stride + i] = gl_mul(x[stride + i], s); x[2 * stride + i] = gl_mul(x[2 * stride + i], s);
    }
}

// power tables of an arbitrary factor, built on the device (bfs_gl_scale: no host tables, no copies, no synchronisation)
__global__ void gl_power_tables_kernel(u64* lo, u64* hi, u32 lo_bits, u32 hi_bits, u64 factor) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (1u << lo_bits)) lo[i] = gl_pow(factor, i);
    if (i < (1u << hi_bits)) hi[i] = gl_pow(factor, (u64)i << lo_bits);
}

__global__ void gl_scale_kernel(const u64* in, u64* out, u64 n, u64 stride, const u64* s_lo, const u64* s_hi, u32 lo_bits) {
    const u64 b = blockIdx.y;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
        out[b * stride + i] = gl_mul(in[b * stride + i], tw_pow(s_lo, s_hi, lo_bits, i));
}

static u32 grid_for(u64 n, u32 block) {
    u64 g = (n + block - 1) / block;
    return (u32)(g > 2048 ? 2048 : (g ? g : 1));
}

int mul_pointwise_launch(const u64* a, const u64* b, u64* out, u64 n, hipStream_t stream) {
    if (!n) return BFS_OK;
    hipLaunchKernelGGL(gl_mul_pointwise_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, a, b, out, n);
    BFS_HIP(hipGetLastError());
    return BFS_OK;
}

int batch_inverse_launch(const u64* in, u64* out, u64 n, hipStream_t stream) {
    if (!n) return BFS_OK;
    // the zero flag lives in pooled pinned host memory that the kernel writes directly: the reference's assert needs the answer
    // now, which costs one stream synchronisation but no copy command and no pinning of pageable memory
    void* h_flag = nullptr;
    void* d_flag = nullptr;
    BFS_TRY(host_alloc(64, &h_flag));
    *(volatile unsigned int*)h_flag = 0;
    if (hipHostGetDevicePointer(&d_flag, h_flag, 0) != hipSuccess) { (void)host_release(h_flag); set_error("hipHostGetDevicePointer failed"); return BFS_ERR_HIP; }
    const u64 per_block = (u64)BINV_T * BINV_E;
    hipLaunchKernelGGL(gl_batch_inverse_kernel, dim3((u32)((n + per_block - 1) / per_block)), dim3(BINV_T), 0, stream, in, out, n, (unsigned int*)d_flag);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    const unsigned int flag = *(volatile unsigned int*)h_flag;
    (void)host_release(h_flag);
    if (e != hipSuccess) { set_error("batch inverse: %s", hipGetErrorString(e)); return BFS_ERR_HIP; }
    if (flag) { set_error("batch inverse does not work when input contains a zero"); return BFS_ERR_ZERO_IN_BATCH_INVERSE; }
    return BFS_OK;
}

int xfe_mul_pointwise_launch(const u64* a, u64 a_stride, const u64* b, u64 b_stride, u64* out, u64 out_stride, u64 n, hipStream_t stream) {
    if (!n) return BFS_OK;
    hipLaunchKernelGGL(xfe_mul_pointwise_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, a, a_stride, b, b_stride, out, out_stride, n);
    BFS_HIP(hipGetLastError());
    return BFS_OK;
}

int xfe_batch_inverse_launch(const u64* in, u64 in_stride, u64* out, u64 out_stride, u64 n, hipStream_t stream) {
    if (!n) return BFS_OK;
    void* w = nullptr;
    BFS_TRY(workspace(8, n * sizeof(u64), stream, &w));
    u64* norm = (u64*)w;
    hipLaunchKernelGGL(xfe_cofactors_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, in, in_stride, out, out_stride, norm, n);
    BFS_HIP(hipGetLastError());
    // a zero element has norm zero: the base field's launch reports it (BFS_ERR_ZERO_IN_BATCH_INVERSE, ntt.py:178-179) and leaves
    // inverse(0) = 0 in its place, so the output of a zero is zero as in extension_field.py:80-83 (xgcd of the zero polynomial)
    const int rc = batch_inverse_launch(norm, norm, n, stream);
    if (rc != BFS_OK && rc != BFS_ERR_ZERO_IN_BATCH_INVERSE) return rc;
    hipLaunchKernelGGL(xfe_scale_by_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, out, out_stride, norm, n);
    BFS_HIP(hipGetLastError());
    return rc;
}

int scale_launch(const u64* in, u64* out, u64 n, u64 stride, u32 batch, u64 factor, hipStream_t stream) {
    if (!n || !batch) return BFS_OK;
    u32 log_n = 0;
    while ((1ull << log_n) < n) ++log_n;
    // two-level power tables of `factor` split at lo_bits (factor^i = lo[i & mask] * hi[i >> lo_bits]), not cached (arbitrary
    // factors would pile up) and built by a small kernel in stream-ordered workspace: nothing here touches the host
    const u32 lo_bits = (log_n + 1) / 2, hi_bits = log_n - lo_bits;
    void* w = nullptr;
    BFS_TRY(workspace(2, ((1ull << lo_bits) + (1ull << hi_bits)) * sizeof(u64), stream, &w));
    u64* d_lo = (u64*)w;
    u64* d_hi = d_lo + (1ull << lo_bits);
    const u32 entries = 1u << lo_bits;           // lo_bits >= hi_bits
    hipLaunchKernelGGL(gl_power_tables_kernel, dim3((entries + 255) / 256), dim3(256), 0, stream, d_lo, d_hi, lo_bits, hi_bits, factor);
    BFS_HIP(hipGetLastError());
    hipLaunchKernelGGL(gl_scale_kernel, dim3(grid_for(n, 256), batch), dim3(256), 0, stream, in, out, n, stride, d_lo, d_hi, lo_bits);
    BFS_HIP(hipGetLastError());
    return BFS_OK;
}

}  // namespace bfs
