// deep.hip -- opening committed polynomials at points outside the FRI domain (include/bfstark_ext.h): the values f_b(z_j) of
// coefficient columns in HBM at up to four points of F_p^3, and the DEEP quotient codeword that ties the values to the committed
// codewords.  The per-thread arithmetic, with the cost argument, is deep_core.hpp; DESIGN.md "Opening at out-of-domain points".
// include/bfstark_open.h adds the same two for opening plans: separate columns of their own lengths evaluated in one call, and the
// quotient of groups of columns that are opened at different points, in one launch.
// include/bfstark_rounds.h adds the quotient of a plan over the columns of several commitments: the same kernel, launched as often as
// the plan needs (deep_core.hpp: deep_rounds_split), every launch after the first accumulating into the output.
//
// The host side is shared as far as the kernels allow.  Both evaluation entries are eval_launches behind their own column checks.  All
// three quotient entries ask the same of domain and codewords (check_domain, check_codewords).  Both PLAN entries are one driver,
// deep_quotient_plan, called with the entry's name and limits: deep_core.hpp's one check of a plan, its split, and per launch its one
// filling of a DeepGroupsArgs.  So a plan within bfsx_deep_quotient_groups' limits is always exactly one launch (every bound of the split
// is one of them), and a launch gets the points its pairs name in order of first appearance: points in another order, or a point no pair
// uses, select the instantiation for the points in use and change no word (field arithmetic is exact); an unused point is still
// checked for being reduced.  bfs_deep_quotient keeps its own argument block and kernel: one group is 1.11-1.17x cheaper there
// (profiles/pcs.md).
// No entry synchronises, copies from the host or allocates outside the stream-ordered pool: the points, weights, constants, column
// tables and plans of a call travel as kernel arguments.
#include "../../include/bfstark_ext.h"
#include "../../include/bfstark_open.h"
#include "../../include/bfstark_rounds.h"
#include "deep_core.hpp"
#include "runtime.hpp"

namespace bfs {

// the table of a launch (deep_core.hpp): block j = point j
__global__ void __launch_bounds__(DEEP_EVAL_T) deep_eval_table_kernel(DeepPoints pts, u64* table) {
    deep_eval_table_entry(pts.z[blockIdx.x], blockIdx.x, threadIdx.x, table);
}

// the sum of the workgroup's 256 elements, in thread 0 (field addition is exact: any order gives the same element)
__device__ __forceinline__ Xfe deep_block_sum(const Xfe& mine, u64* red) {
    const u32 t = threadIdx.x;
    __syncthreads();                                      // (the previous sum has been read)
    red[t] = mine.c[0]; red[DEEP_EVAL_T + t] = mine.c[1]; red[2 * DEEP_EVAL_T + t] = mine.c[2];
    __syncthreads();
    for (u32 d = DEEP_EVAL_T / 2; d > 0; d >>= 1) {
        if (t < d) {
            red[t] = gl_add(red[t], red[t + d]);
            red[DEEP_EVAL_T + t] = gl_add(red[DEEP_EVAL_T + t], red[DEEP_EVAL_T + t + d]);
            red[2 * DEEP_EVAL_T + t] = gl_add(red[2 * DEEP_EVAL_T + t], red[2 * DEEP_EVAL_T + t + d]);
        }
        __syncthreads();
    }
    return Xfe{{red[0], red[DEEP_EVAL_T], red[2 * DEEP_EVAL_T]}};
}

// a workgroup's share of one column: out[3 j ..] = its part of f(z_j) without its z_j^(B block)
template <int K>
__device__ __forceinline__ void deep_eval_partial_block(const u64* col, u64 n, u32 block, const u64* table, u64* out, u32 out_step) {
    __shared__ u64 steps[K * DEEP_EVAL_S * 3];
    __shared__ u64 red[3 * DEEP_EVAL_T];
    const u32 t = threadIdx.x;
    for (u32 w = t; w < (u32)K * DEEP_EVAL_S * 3; w += DEEP_EVAL_T) steps[w] = table[DEEP_EVAL_STEPS_AT + w];
    __syncthreads();
    Xfe mine[K];
    deep_eval_thread<K>(col, n, block, t, steps, table, mine);
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const Xfe total = deep_block_sum(mine[j], red);
        if (t == 0) { out[(size_t)j * out_step] = total.c[0]; out[(size_t)j * out_step + 1] = total.c[1]; out[(size_t)j * out_step + 2] = total.c[2]; }
    }
}

// `blocks` partial sums at `partial`, each scaled by (z_j^B)^block, added into out[0..3)
__device__ __forceinline__ void deep_eval_combine_block(const u64* partial, u32 blocks, u32 j, const u64* table, u64* out) {
    __shared__ u64 red[3 * DEEP_EVAL_T];
    const u32 t = threadIdx.x;
    const Xfe zb = deep_eval_block_power(table, j);
    Xfe acc{{0, 0, 0}};
    for (u32 p = t; p < blocks; p += DEEP_EVAL_T) acc = xfe_add(acc, xfe_mul(xfe_load3(partial + (u64)p * 3), xfe_pow_small(zb, p)));
    const Xfe total = deep_block_sum(acc, red);
    if (t == 0) { out[0] = total.c[0]; out[1] = total.c[1]; out[2] = total.c[2]; }
}

// launch 1: grid (blocks, batch); partial[((b * K + j) * blocks + block) * 3 ..] = the workgroup's share of f_b(z_j)
template <int K>
__global__ void __launch_bounds__(DEEP_EVAL_T) deep_eval_partial_kernel(const u64* coeffs, u64 n, u64 in_stride, const u64* table, u64* partial) {
    deep_eval_partial_block<K>(coeffs + (u64)blockIdx.y * in_stride, n, blockIdx.x, table,
                               partial + deep_eval_partial_at(blockIdx.y, K, 0, gridDim.x, blockIdx.x), gridDim.x * 3);
}

// launch 2: block (b * k + j) adds the `blocks` partial sums of f_b(z_j)
__global__ void __launch_bounds__(DEEP_EVAL_T) deep_eval_combine_kernel(const u64* partial, u32 blocks, u32 k, const u64* table, u64* out) {
    deep_eval_combine_block(partial + (u64)blockIdx.x * blocks * 3, blocks, blockIdx.x % k, table, out + (u64)blockIdx.x * 3);
}

// the same two launches over separate columns (deep_core.hpp): grid (blocks of the longest column, columns); a workgroup past the
// end of its column leaves as a whole, and the slots it would have filled are never read
template <int K>
__global__ void __launch_bounds__(DEEP_EVAL_T) deep_eval_columns_partial_kernel(DeepEvalColumns cols, const u64* table, u64* partial) {
    const u32 b = blockIdx.y, n = cols.n[b];
    if (blockIdx.x >= deep_eval_blocks(n)) return;
    deep_eval_partial_block<K>(cols.col[b], n, blockIdx.x, table, partial + deep_eval_partial_at(b, K, 0, gridDim.x, blockIdx.x), gridDim.x * 3);
}

__global__ void __launch_bounds__(DEEP_EVAL_T) deep_eval_columns_combine_kernel(DeepEvalColumns cols, const u64* partial, u32 row_blocks, u32 k,
                                                                                const u64* table, u64* out) {
    const u32 b = blockIdx.x / k, j = blockIdx.x % k;
    deep_eval_combine_block(partial + deep_eval_partial_at(b, k, j, row_blocks, 0), deep_eval_blocks(cols.n[b]), j, table, out + (u64)blockIdx.x * 3);
}

template <int K>
__global__ void __launch_bounds__(DEEP_Q_T) deep_quotient_kernel(DeepQuotientArgs a, u64* out, u64 out_stride) {
    const u64 first = (u64)blockIdx.x * (DEEP_Q_T * DEEP_Q_E) + threadIdx.x;
    u64 idx[DEEP_Q_E];
#pragma unroll
    for (u32 e = 0; e < DEEP_Q_E; ++e) idx[e] = first + (u64)e * DEEP_Q_T;
    Xfe g[DEEP_Q_E];
    deep_quotient_thread<K>(a, idx, g);
#pragma unroll
    for (u32 e = 0; e < DEEP_Q_E; ++e) {
        if (idx[e] < a.n) { out[idx[e]] = g[e].c[0]; out[out_stride + idx[e]] = g[e].c[1]; out[2 * out_stride + idx[e]] = g[e].c[2]; }
    }
}

// one launch for a whole opening plan (deep_core.hpp): NP distinct points, E = deep_groups_e(NP) points of the domain per thread
static_assert(sizeof(DeepGroupsArgs) + 2 * sizeof(u64) <= 4096, "the plan must fit the kernel-argument block");
static_assert(sizeof(DeepEvalColumns) + 4 * sizeof(u64) <= 4096, "the column table must fit the kernel-argument block");

// ACC: a later launch of an opening across commitments (deep_core.hpp): the sum starts from what `out` holds
template <int NP, bool ACC>
__global__ void __launch_bounds__(DEEP_G_T) deep_groups_kernel(DeepGroupsArgs a, u64* out, u64 out_stride) {
    constexpr int E = (int)deep_groups_e(NP);
    const u64 first = (u64)blockIdx.x * (DEEP_G_T * E) + threadIdx.x;
    u64 idx[E];
#pragma unroll
    for (int e = 0; e < E; ++e) idx[e] = first + (u64)e * DEEP_G_T;
    Xfe g[E];
    if constexpr (ACC) {
        Xfe start[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const u64 at = idx[e] < a.n ? idx[e] : 0;      // (a thread past the end reads point 0 and stores nothing)
            start[e] = Xfe{{out[at], out[out_stride + at], out[2 * out_stride + at]}};
        }
        deep_groups_thread_from<NP, E>(a, idx, start, g);
    } else {
        deep_groups_thread<NP, E>(a, idx, g);
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (idx[e] < a.n) { out[idx[e]] = g[e].c[0]; out[out_stride + idx[e]] = g[e].c[1]; out[2 * out_stride + idx[e]] = g[e].c[2]; }
    }
}

static bool canonical3(const u64* w) { return w[0] < GL_P && w[1] < GL_P && w[2] < GL_P; }

static bool overlaps(const void* a, u64 a_bytes, const void* b, u64 b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}

// what the two evaluation entries share once their columns are checked: the points, the scratch block (the table, then 3 k words per
// partial sum of a point: `sums` = columns * workgroups of the longest), the table's launch, the entry's own pair of launches
// -- partial(K, table, partial sums), combine(table, partial sums) -- and the release
template <class Partial, class Combine>
static int eval_launches(const char* entry, const u64* h_points, u32 k, u64 sums, hipStream_t stream, Partial&& partial, Combine&& combine) {
    if (k < 1 || k > DEEP_MAX_POINTS) { set_error("%s: the number of points must be 1..%u (got %u)", entry, DEEP_MAX_POINTS, k); return BFS_ERR_BAD_ARG; }
    DeepPoints pts{};
    for (u32 j = 0; j < k; ++j) {
        if (!canonical3(h_points + 3 * j)) { set_error("%s: point %u is not reduced", entry, j); return BFS_ERR_BAD_ARG; }
        pts.z[j] = xfe_load3(h_points + 3 * j);
    }
    void* scratch = nullptr;
    BFS_TRY(device_alloc((DEEP_EVAL_TABLE_WORDS + sums * k * 3) * sizeof(u64), stream, &scratch));
    u64* table = (u64*)scratch;
    u64* sums_at = table + DEEP_EVAL_TABLE_WORDS;
    hipLaunchKernelGGL(deep_eval_table_kernel, dim3(k), dim3(DEEP_EVAL_T), 0, stream, pts, table);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        (void)deep_with_count<DEEP_MAX_POINTS>(k, [&](auto kk) -> int { partial(kk, (const u64*)table, sums_at); return BFS_OK; });
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        combine((const u64*)table, (const u64*)sums_at);
        e = hipGetLastError();
    }
    (void)device_release(scratch, stream);                // stream-ordered: the launches above are ahead of whoever gets the block next
    if (e != hipSuccess) { set_error("%s: %s", entry, hipGetErrorString(e)); return BFS_ERR_HIP; }
    return BFS_OK;
}

// what the three quotient entries ask of the domain and of lambda
static int check_domain(const char* entry, u32 log_n, u64 limb_stride, u64 out_stride, u64 offset, u64 omega, const u64* h_lambda) {
    if (log_n < 1 || log_n > 24) { set_error("%s: log_n must be 1..24 (got %u)", entry, log_n); return BFS_ERR_BAD_ARG; }
    const u64 n = 1ull << log_n;
    if (limb_stride < n || out_stride < n) { set_error("%s: a stride shorter than the domain", entry); return BFS_ERR_BAD_ARG; }
    if (offset == 0 || offset >= GL_P || omega >= GL_P) { set_error("%s: offset or omega is not a reduced non-zero value", entry); return BFS_ERR_BAD_ARG; }
    if (gl_pow(omega, n) != 1 || gl_pow(omega, n / 2) == 1) { set_error("omega does not have the right order"); return BFS_ERR_NOT_ROOT; }
    if (!canonical3(h_lambda)) { set_error("%s: lambda is not reduced", entry); return BFS_ERR_BAD_ARG; }
    return BFS_OK;
}

// ... and of the codewords: none null, none under the output
static int check_codewords(const char* entry, const bfs_row_column* h_columns, u32 m, u64 limb_stride, u64 n, const u64* d_out, u64 out_stride) {
    for (u32 p = 0; p < m; ++p) {
        const bfs_row_column& c = h_columns[p];
        if (!c.d_values) { set_error("%s: codeword %u is null", entry, p); return BFS_ERR_BAD_ARG; }
        if (overlaps(d_out, (2 * out_stride + n) * 8, c.d_values, (c.is_ext ? 2 * limb_stride + n : n) * 8)) { set_error("%s: d_out overlaps codeword %u", entry, p); return BFS_ERR_BAD_ARG; }
    }
    return BFS_OK;
}

// THE driver of both plan entries: the plan against the entry's limits (deep_plan_check), the domain, the words, the codewords; then the
// split into launches (deep_rounds_split: always one launch within DEEP_G_LIMITS) and per launch deep_rounds_args and the kernel
static int deep_quotient_plan(const char* entry, const DeepPlanLimits& limits, const bfs_row_column* h_columns, u32 m, u64 limb_stride, u32 log_n,
                              u64 offset, u64 omega, const u32* h_group_columns, const u32* h_group_pairs, u32 n_groups, const u64* h_points,
                              u32 n_points, const u32* h_pair_point, const u64* h_pair_values, const u64* h_lambda, u64* d_out, u64 out_stride,
                              u32* h_launches, hipStream_t stream) {
    if (!h_columns || !h_group_columns || !h_group_pairs || !h_points || !h_pair_point || !h_pair_values || !h_lambda || !d_out) {
        set_error("%s: null argument", entry); return BFS_ERR_BAD_ARG;
    }
    char why[96];
    if (!deep_plan_check(limits, m, h_group_columns, h_group_pairs, n_groups, n_points, h_pair_point, why)) { set_error("%s: %s", entry, why); return BFS_ERR_BAD_ARG; }
    BFS_TRY(check_domain(entry, log_n, limb_stride, out_stride, offset, omega, h_lambda));
    const u64 n = 1ull << log_n;
    for (u32 p = 0; p < n_points; ++p) {                  // (every point of the plan, whether a pair names it or not)
        if (!canonical3(h_points + 3 * p)) { set_error("%s: point %u is not reduced", entry, p); return BFS_ERR_BAD_ARG; }
    }
    u32 pairs = 0;
    for (u32 g = 0; g < n_groups; ++g) pairs += h_group_pairs[g];
    for (u32 q = 0; q < pairs; ++q) {
        if (!canonical3(h_pair_values + 3 * q)) { set_error("%s: value %u is not reduced", entry, q); return BFS_ERR_BAD_ARG; }
    }
    BFS_TRY(check_codewords(entry, h_columns, m, limb_stride, n, d_out, out_stride));
    const u64* col[DEEP_R_COLUMNS];
    int is_ext[DEEP_R_COLUMNS];
    for (u32 c = 0; c < m; ++c) { col[c] = h_columns[c].d_values; is_ext[c] = h_columns[c].is_ext != 0; }
    DeepRoundsLaunch launches[DEEP_R_GROUPS];
    const u32 count = deep_rounds_split(h_group_columns, h_group_pairs, n_groups, h_pair_point, launches);
    if (h_launches) *h_launches = count;
    DeepGroupsArgs common{};
    common.limb_stride = limb_stride; common.n = n; common.offset = offset;
    BFS_TRY(ntt_power_tables(omega, log_n, &common.w_lo, &common.w_hi, &common.lo_bits));
    const Xfe lambda = xfe_load3(h_lambda);
    Xfe scale{{1, 0, 0}};                                 // lambda^base of the next pair, across the launches
    for (u32 l = 0; l < count; ++l) {
        DeepGroupsArgs a = common;
        deep_rounds_args(a, launches[l], col, is_ext, h_group_columns, h_group_pairs, h_points, h_pair_point, h_pair_values, lambda, scale);
        const u64 share = (u64)DEEP_G_T * deep_groups_e(launches[l].n_points);
        const u32 grid = (u32)((n + share - 1) / share);
        (void)deep_with_count<DEEP_G_POINTS>(launches[l].n_points, [&](auto np) -> int {
            // the first launch writes d_out and never reads it; every later one starts from what the one before left there
            if (l == 0) hipLaunchKernelGGL((deep_groups_kernel<decltype(np)::value, false>), dim3(grid), dim3(DEEP_G_T), 0, stream, a, d_out, out_stride);
            else hipLaunchKernelGGL((deep_groups_kernel<decltype(np)::value, true>), dim3(grid), dim3(DEEP_G_T), 0, stream, a, d_out, out_stride);
            return BFS_OK;
        });
        BFS_HIP(hipGetLastError());
    }
    return BFS_OK;
}

}  // namespace bfs

using namespace bfs;

extern "C" int bfs_poly_eval_points(const uint64_t* d_coeffs, uint64_t n_coeffs, uint64_t in_stride, uint32_t batch, const uint64_t* h_points,
                                    uint32_t k, uint64_t* d_out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!d_coeffs || !h_points || !d_out) { set_error("bfs_poly_eval_points: null argument"); return BFS_ERR_BAD_ARG; }
    if (n_coeffs < 1 || n_coeffs > (1ull << 24)) { set_error("bfs_poly_eval_points: n_coeffs must be 1..2^24 (got %llu)", (unsigned long long)n_coeffs); return BFS_ERR_BAD_ARG; }
    if (batch < 1 || batch > 65535) { set_error("bfs_poly_eval_points: batch must be 1..65535 (got %u)", batch); return BFS_ERR_BAD_ARG; }
    if (batch > 1 && in_stride < n_coeffs) { set_error("bfs_poly_eval_points: in_stride < n_coeffs"); return BFS_ERR_BAD_ARG; }
    const u32 blocks = deep_eval_blocks(n_coeffs);
    const u64 results = (u64)batch * k;
    if (overlaps(d_out, results * 24, d_coeffs, ((u64)(batch - 1) * in_stride + n_coeffs) * 8)) { set_error("bfs_poly_eval_points: d_out overlaps the coefficients"); return BFS_ERR_BAD_ARG; }
    return eval_launches("bfs_poly_eval_points", h_points, k, (u64)batch * blocks, stream,
        [&](auto kk, const u64* table, u64* partial) {
            hipLaunchKernelGGL((deep_eval_partial_kernel<decltype(kk)::value>), dim3(blocks, batch), dim3(DEEP_EVAL_T), 0, stream, d_coeffs, n_coeffs, in_stride, table, partial);
        },
        [&](const u64* table, const u64* partial) {
            hipLaunchKernelGGL(deep_eval_combine_kernel, dim3((u32)results), dim3(DEEP_EVAL_T), 0, stream, partial, blocks, k, table, d_out);
        });
}

extern "C" int bfsx_poly_eval_columns(const bfsx_eval_column* h_columns, uint32_t count, const uint64_t* h_points, uint32_t k, uint64_t* d_out,
                                      void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h_columns || !h_points || !d_out) { set_error("bfsx_poly_eval_columns: null argument"); return BFS_ERR_BAD_ARG; }
    if (count < 1 || count > DEEP_EVAL_MAX_COLUMNS) { set_error("bfsx_poly_eval_columns: 1..%u columns (got %u)", DEEP_EVAL_MAX_COLUMNS, count); return BFS_ERR_BAD_ARG; }
    const u64 results = (u64)count * k;
    DeepEvalColumns cols{};
    u32 row_blocks = 0;
    for (u32 b = 0; b < count; ++b) {
        const bfsx_eval_column& c = h_columns[b];
        if (!c.d_coeffs) { set_error("bfsx_poly_eval_columns: column %u is null", b); return BFS_ERR_BAD_ARG; }
        if (c.n_coeffs < 1 || c.n_coeffs > (1ull << 24)) { set_error("bfsx_poly_eval_columns: column %u: n_coeffs must be 1..2^24 (got %llu)", b, (unsigned long long)c.n_coeffs); return BFS_ERR_BAD_ARG; }
        if (overlaps(d_out, results * 24, c.d_coeffs, c.n_coeffs * 8)) { set_error("bfsx_poly_eval_columns: d_out overlaps column %u", b); return BFS_ERR_BAD_ARG; }
        cols.col[b] = c.d_coeffs;
        cols.n[b] = (u32)c.n_coeffs;
        if (deep_eval_blocks(c.n_coeffs) > row_blocks) row_blocks = deep_eval_blocks(c.n_coeffs);
    }
    return eval_launches("bfsx_poly_eval_columns", h_points, k, (u64)count * row_blocks, stream,
        [&](auto kk, const u64* table, u64* partial) {
            hipLaunchKernelGGL((deep_eval_columns_partial_kernel<decltype(kk)::value>), dim3(row_blocks, count), dim3(DEEP_EVAL_T), 0, stream, cols, table, partial);
        },
        [&](const u64* table, const u64* partial) {
            hipLaunchKernelGGL(deep_eval_columns_combine_kernel, dim3((u32)results), dim3(DEEP_EVAL_T), 0, stream, cols, partial, row_blocks, k, table, d_out);
        });
}

// one group at up to four points: its own argument block and kernel (fewer registers than the plan's kernel, profiles/pcs.md)
extern "C" int bfs_deep_quotient(const bfs_row_column* h_columns, uint32_t m, uint64_t limb_stride, uint32_t log_n, uint64_t offset, uint64_t omega,
                                 const uint64_t* h_points, const uint64_t* h_values, uint32_t k, const uint64_t h_lambda[3], uint64_t* d_out,
                                 uint64_t out_stride, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* entry = "bfs_deep_quotient";
    if (!h_columns || !h_points || !h_values || !h_lambda || !d_out) { set_error("bfs_deep_quotient: null argument"); return BFS_ERR_BAD_ARG; }
    if (m < 1 || m > DEEP_MAX_COLUMNS) { set_error("bfs_deep_quotient: 1..%u codewords (got %u)", DEEP_MAX_COLUMNS, m); return BFS_ERR_BAD_ARG; }
    if (k < 1 || k > DEEP_MAX_POINTS) { set_error("bfs_deep_quotient: the number of points must be 1..%u (got %u)", DEEP_MAX_POINTS, k); return BFS_ERR_BAD_ARG; }
    BFS_TRY(check_domain(entry, log_n, limb_stride, out_stride, offset, omega, h_lambda));
    const u64 n = 1ull << log_n;
    BFS_TRY(check_codewords(entry, h_columns, m, limb_stride, n, d_out, out_stride));
    DeepQuotientArgs a{};
    a.m = m; a.limb_stride = limb_stride; a.n = n; a.offset = offset;
    const Xfe lambda = xfe_load3(h_lambda);
    Xfe power{{1, 0, 0}};                                 // lambda^p
    for (u32 p = 0; p < m; ++p) {
        a.col[p] = h_columns[p].d_values;
        if (h_columns[p].is_ext) a.ext_mask |= 1u << p;
        lazy_weight_matrix(power, a.weight[p]);
        power = xfe_mul(power, lambda);
    }
    Xfe scale{{1, 0, 0}};                                 // lambda^(j m)
    for (u32 j = 0; j < k; ++j) {
        if (!canonical3(h_points + 3 * j) || !canonical3(h_values + 3 * j)) { set_error("bfs_deep_quotient: point or value %u is not reduced", j); return BFS_ERR_BAD_ARG; }
        deep_point_consts(a.pt[j], xfe_load3(h_points + 3 * j), scale, xfe_load3(h_values + 3 * j));
        scale = xfe_mul(scale, power);
    }
    BFS_TRY(ntt_power_tables(omega, log_n, &a.w_lo, &a.w_hi, &a.lo_bits));
    const u32 grid = (u32)((n + DEEP_Q_T * DEEP_Q_E - 1) / (DEEP_Q_T * DEEP_Q_E));
    (void)deep_with_count<DEEP_MAX_POINTS>(k, [&](auto kk) -> int {
        hipLaunchKernelGGL((deep_quotient_kernel<decltype(kk)::value>), dim3(grid), dim3(DEEP_Q_T), 0, stream, a, d_out, out_stride);
        return BFS_OK;
    });
    BFS_HIP(hipGetLastError());
    return BFS_OK;
}

extern "C" int bfsx_deep_quotient_groups(const bfs_row_column* h_columns, uint32_t m, uint64_t limb_stride, uint32_t log_n, uint64_t offset,
                                         uint64_t omega, const uint32_t* h_group_columns, const uint32_t* h_group_pairs, uint32_t n_groups,
                                         const uint64_t* h_points, uint32_t n_points, const uint32_t* h_pair_point, const uint64_t* h_pair_values,
                                         const uint64_t h_lambda[3], uint64_t* d_out, uint64_t out_stride, void* stream) {
    return deep_quotient_plan("bfsx_deep_quotient_groups", DEEP_G_LIMITS, h_columns, m, limb_stride, log_n, offset, omega, h_group_columns, h_group_pairs,
                              n_groups, h_points, n_points, h_pair_point, h_pair_values, h_lambda, d_out, out_stride, nullptr, (hipStream_t)stream);
}

extern "C" int bfsr_deep_quotient_rounds(const bfs_row_column* h_columns, uint32_t m, uint64_t limb_stride, uint32_t log_n, uint64_t offset,
                                         uint64_t omega, const uint32_t* h_group_columns, const uint32_t* h_group_pairs, uint32_t n_groups,
                                         const uint64_t* h_points, uint32_t n_points, const uint32_t* h_pair_point, const uint64_t* h_pair_values,
                                         const uint64_t h_lambda[3], uint64_t* d_out, uint64_t out_stride, uint32_t* h_launches, void* stream) {
    return deep_quotient_plan("bfsr_deep_quotient_rounds", DEEP_R_LIMITS, h_columns, m, limb_stride, log_n, offset, omega, h_group_columns, h_group_pairs,
                              n_groups, h_points, n_points, h_pair_point, h_pair_values, h_lambda, d_out, out_stride, h_launches, (hipStream_t)stream);
}
