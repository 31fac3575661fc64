// runtime.hpp -- host-side plumbing shared by the translation units of libbfstark_hip.so:
// error reporting (bfs_last_error), HIP call checking, cached device tables and per-stream scratch space.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "ntt_plan.hpp"

namespace bfs {

void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
const char* last_error();

#define BFS_HIP(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) {                                                                         \
            ::bfs::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return BFS_ERR_HIP;                                                                         \
        }                                                                                               \
    } while (0)

#define BFS_TRY(expr)            \
    do {                         \
        int rc_ = (expr);        \
        if (rc_) return rc_;     \
    } while (0)

// grow-only scratch buffer keyed by (device, stream, slot); contents are only valid within one API call
int workspace(int slot, size_t bytes, hipStream_t stream, void** out);
int workspace_release(int slot, hipStream_t stream);
bool workspace_peek(int slot, hipStream_t stream, void** ptr, size_t* bytes);   // the slot's buffer if it exists (no allocation)

// Pooled HBM and pinned-host memory.  hipMalloc / hipFree cost 50-500 us and hipFree synchronises the device, which at
// 288 GB of HBM is the wrong trade: freed blocks go back to a size-class free list (8 classes per octave above 1 MiB,
// powers of two below) and are handed out again without touching the driver.  Reuse is STREAM-ORDERED, like
// hipMallocAsync: a block released on stream S may be handed to work on S immediately (earlier work on S still reading
// it is ahead in the queue); a request from another stream -- or from the stream-less bfs_malloc -- synchronises S first.
// `NO_STREAM` as the release stream means "the device was idle when the block came back".
static const hipStream_t NO_STREAM = (hipStream_t)(uintptr_t)-1;
int device_alloc(size_t bytes, hipStream_t stream, void** out);
int device_release(void* ptr, hipStream_t stream);
int device_pool_trim();                                     // hipFree every cached block (synchronises the device)
void device_pool_stats(size_t* live_bytes, size_t* cached_bytes);
int host_alloc(size_t bytes, void** out);                   // pinned, pooled the same way (no stream semantics: callers copy synchronously)
int host_release(void* ptr);

// Blocking copies between host and HBM.  Large pageable host buffers are bounced through two pinned 8 MiB buffers from
// the host pool (the memcpy of chunk k+1 overlaps the DMA of chunk k) instead of letting the runtime pin the user pages:
// that path measured ~1 GB/s, and the unpinning afterwards stalls later kernel dispatches for ~25 ms.
int copy_h2d(void* d, const void* h, size_t bytes, hipStream_t stream);
int copy_d2h(void* h, const void* d, size_t bytes, hipStream_t stream);

// The library's second stream next to a caller's stream, with the events that fork it from that stream and join it back (the NTT's
// column pipeline).  One per (device, caller's stream), created the first time it is asked for and kept until stream_retire -- not
// one per device: work of two callers queued on one shared helper would make either caller's stream wait for whatever the OTHER
// one's stream is waiting for.  Threads that call on different streams share nothing; threads that call on the SAME stream share
// the pair, and an event recorded twice before it is waited for only makes the wait cover more.
struct StreamPair {
    hipStream_t helper;
    hipEvent_t fork, join;
};
int stream_pair(hipStream_t stream, StreamPair* out);

// a stream is about to be destroyed: wait for it, free its scratch buffers and its second stream, forget it in the pools
int stream_retire(hipStream_t stream);

// upload a host table once and keep it (keyed by caller-chosen values; the cache starts over after 4096 entries, runtime.cpp)
int cached_table(uint64_t key_a, uint64_t key_b, uint64_t key_c, const u64* host, size_t count, const u64** d_out);
bool cached_table_lookup(uint64_t key_a, uint64_t key_b, uint64_t key_c, const u64** d_out);

// ---- FRI rounds on small codewords, one launch (merkle.hip: fri_round_quad_kernel) ----
// A round folds its codeword by a = 2^k, k = log2_folding in {1, 2, 3}: k successive split-and-fold steps (fri.py:127-128) with the
// challenges alpha, alpha^2, alpha^4, offset and omega squared between the steps.  Output c, c < half = n / a, depends on the a inputs
// in[c + m * half]; step j pairs v[m] with v[m + h], h = 2^(k-1-j), at abscissa offset^(2^j) * omega^(2^j * (c + m * half)), and
// omega^half is a primitive a-th root of unity zeta.  So the factor 2^-1 / x of pair m in step j is
//     scal[off_j + m] * (omega^-c)^(2^j),   scal[off_j + m] = 2^-1 * offset^-(2^j) * zeta^-(m * 2^j),   off_j = a - 2^(k-j)
// -- 1, 3 or 7 kernel-argument constants -- and the thread looks up omega^-c once.
struct FriFoldArgs {
    const u64* in;             // previous round's codeword (null: this round's codeword is already at cw)
    u64 in_stride, half;       // half = length of this round's codeword
    Xfe alpha[3];              // fri.py:120 and its squares: alpha^(2^j), j < k
    u64 scal[7];               // see above; k = 1: scal[0] = 2^-1 * offset_r^-1
    const u64* winv_lo;        // two-level powers of the round-0 omega^-1
    const u64* winv_hi;
    u32 lo_bits, round_shift;  // omega_r = omega_0^(2^round_shift)
    u32 log2_folding;          // k
};
// host side: the constants of one fold by 2^k of a codeword of length n over offset * <omega> (omega of order n)
inline void fri_fold_constants(FriFoldArgs& f, u32 k, u64 n, const Xfe& alpha, u64 offset, u64 omega) {
    f.log2_folding = k;
    f.half = n >> k;
    f.alpha[0] = alpha;
    for (u32 j = 1; j < 3; ++j) f.alpha[j] = j < k ? xfe_mul(f.alpha[j - 1], f.alpha[j - 1]) : Xfe{{0, 0, 0}};
    u64 gj = gl_mul(gl_inv(2), gl_inv(offset));                 // 2^-1 * offset^-(2^j)
    u64 zj = k > 1 ? gl_pow(gl_inv(omega), f.half) : 1;          // zeta^-(2^j)
    u32 off = 0;
    for (u32 j = 0; j < k; ++j) {
        const u32 h = 1u << (k - 1 - j);
        u64 z = 1;
        for (u32 m = 0; m < h; ++m) { f.scal[off + m] = gl_mul(gj, z); z = gl_mul(z, zj); }
        off += h;
        gj = gl_mul(gl_mul(gj, gj), 2);                          // (2^-1 g)^2 * 2 = 2^-1 g^2
        zj = gl_sqr(zj);
    }
    for (; off < 7; ++off) f.scal[off] = 0;
}

BFS_HD u64 gl_half(u64 x) { return (x >> 1) + ((x & 1) ? 0x7FFFFFFF80000001ULL : 0); }  // x / 2 mod p

// one output element of a fold by 2^K: element i of the folded codeword, from f.in[i + m * f.half], m < 2^K (limb-major, stride
// f.in_stride).  The K steps run in registers; K = 1 is fri.py:127-128 as it stands:
//     out[i] = 2^-1 * ((1 + alpha/x_i) * a + (1 - alpha/x_i) * b) = (a + b)/2 + alpha * (2^-1 * offset^-1 * omega^-i) * (a - b)
template <int K>
BFS_HD Xfe fri_fold_point(const FriFoldArgs& f, u64 i) {
    constexpr int A = 1 << K;
    Xfe v[A];
    BFS_UNROLL
    for (int m = 0; m < A; ++m) {
        const u64 at = (u64)m * f.half + i;
        v[m] = Xfe{{f.in[at], f.in[f.in_stride + at], f.in[2 * f.in_stride + at]}};
    }
    u64 w = tw_pow(f.winv_lo, f.winv_hi, f.lo_bits, i << f.round_shift);    // omega_r^-i
    int off = 0;
    BFS_UNROLL
    for (int j = 0; j < K; ++j) {
        const int h = 1 << (K - 1 - j);
        BFS_UNROLL
        for (int m = 0; m < h; ++m) {
            const u64 s = gl_mul(f.scal[off + m], w);
            const Xfe beta = xfe_scale(f.alpha[j], s);
            const Xfe sum = xfe_add(v[m], v[m + h]), diff = xfe_sub(v[m], v[m + h]);
            const Xfe prod = xfe_mul(beta, diff);
            v[m] = Xfe{{gl_add(gl_half(sum.c[0]), prod.c[0]), gl_add(gl_half(sum.c[1]), prod.c[1]), gl_add(gl_half(sum.c[2]), prod.c[2])}};
        }
        off += h;
        if (j + 1 < K) w = gl_sqr(w);
    }
    return v[0];
}
// a runtime log2_folding in 1..3 as the compile-time K of the kernels: returns fn(std::integral_constant<int, K>()), the launch of the instance
template <class Fn>
inline int with_fold_factor(u32 log2_folding, Fn&& fn) {
    switch (log2_folding) {
    case 1: return fn(std::integral_constant<int, 1>());
    case 2: return fn(std::integral_constant<int, 2>());
    case 3: return fn(std::integral_constant<int, 3>());
    default: set_error("internal: fold by 2^%u", log2_folding); return BFS_ERR_BAD_ARG;
    }
}
// levels above the leaves of a tree over n leaves: its leaf level has 2^tree_depth(n) slots
inline u32 tree_depth(u64 n) {
    u32 depth = 0;
    while ((1ull << depth) < n) ++depth;
    return depth;
}
constexpr u64 FRI_FUSED_MAX = 16384;     // up to 256 workgroups of 64 leaves (their roots: one top kernel)
int merkle_build_xfe_fold_launch(const FriFoldArgs& fold, u64* d_cw, u64 cw_stride, u64 n, u64* d_nodes, hipStream_t stream, u64* root_out, u64 seq);
int fri_round_fused_launch(const FriFoldArgs& fold, u64* d_cw, u64 cw_stride, u64 n, u64* d_nodes, hipStream_t stream, u64* root_out, u64 seq);

// ---- internal entry points (device pointers, current device) ----
// ntt.hip.  One bfs_gl_ntt call of at most 65535 transforms, as the pass runner and the route code see it (log_n is the plan's)
struct NttCall {
    const u64* in;
    u64 n_in, in_stride;
    u64* out;
    u64 out_stride;
    u32 batch;
    u64 root, shift, post_scale;
    u32 streaming;                                    // non-temporal data accesses (ntt_core.hpp)
    hipStream_t stream;
};
constexpr u64 NTT_STREAMING_BYTES = 128ull << 20;     // one 2^24-point column (128 MiB) still runs out of the Infinity Cache, two do not
int ntt_launch(const u64* d_in, u64 n_in, u64 in_stride, u64* d_out, u64 out_stride, u32 log_n, u32 batch, u64 root,
               u64 shift, u64 post_scale, hipStream_t stream);
// steps first..last of the call's schedule (ntt_plan.hpp: ntt_make_schedule); mid: the intermediate buffer of passes 0 and 1, or null
int ntt_run_steps(const NttCall& c, const NttPlan& p, u64* mid, u32 first, u32 last);
// two-level power tables of `root` (order 2^log_n): root^e = lo[e & mask] * hi[e >> lo_bits]
int ntt_power_tables(u64 root, u32 log_n, const u64** lo, const u64** hi, u32* lo_bits);
// the environment switches of the transform, each read once per process
constexpr int NTT_ROUTE_CANDIDATES = 3;
constexpr int NTT_ROUTE_DIRECT = -1;                  // a route: direct, or k >= 0 through candidate buffer k
enum class NttRouteMode { Remembered, Auto, Forced };
enum class NttPipeline { Off, BySize, Forced };
constexpr u64 NTT_PIPELINE_MIN_BYTES = 64ull << 20;   // the column pipeline (ntt.hip: ntt_run_columns): bytes of ONE transform's output
constexpr u64 NTT_PIPELINE_MAX_BYTES = 128ull << 20;
struct NttEnv {
    NttRouteMode route_mode;      // BFS_NTT_WS_PROBE unset: routes come from bfs_ntt_tune only; "auto" / "1": bfs_gl_ntt tunes a pair itself the third
    int forced_route;             //   time it sees it; "0" / "direct" / "buffer0..2": Forced, this route for every large transform and tune a no-op
    bool probe_log;               // BFS_NTT_WS_PROBE_LOG=1: the route measurements go to stderr
    int force_streaming;          // BFS_NTT_STREAMING=0 / 1 forces the choice (A/B, tools/ab_ntt.sh); -1: by size
    bool allow_expand;            // BFS_NTT_EXPAND=0: zero-padded transforms take the plain plan too
    bool plan_log;                // BFS_NTT_PLAN_LOG: two stderr lines per tiled call, the plan and the route it took
    NttPipeline pipeline;         // BFS_NTT_PIPELINE=0 / 1 / force: the column pipeline never / by size (default) / for every multi-pass batch
};
const NttEnv& ntt_env();

// ntt_route.cpp: where pass 0 of a large out-of-place transform writes
constexpr int NTT_ROUTE_SLOT0 = 16;                   // workspace slots 16.. hold the candidate buffers
int ntt_route(const NttCall& c, const NttPlan& p, int* route);
int ntt_route_probe_info(float* us, int* route, unsigned long long* probes);
int ntt_tune(const u64* d_in, u64 in_stride, u64* d_out, u64 out_stride, u32 log_n, u32 batch, u64 root, hipStream_t stream, int* route_out);
size_t ntt_route_forget_range(const void* lo, size_t bytes, bool may_free);
void ntt_route_trim();

// pointwise.hip
int mul_pointwise_launch(const u64* a, const u64* b, u64* out, u64 n, hipStream_t stream);
int batch_inverse_launch(const u64* in, u64* out, u64 n, hipStream_t stream);
int scale_launch(const u64* in, u64* out, u64 n, u64 stride, u32 batch, u64 factor, hipStream_t stream);
int xfe_mul_pointwise_launch(const u64* a, u64 a_stride, const u64* b, u64 b_stride, u64* out, u64 out_stride, u64 n, hipStream_t stream);
int xfe_batch_inverse_launch(const u64* in, u64 in_stride, u64* out, u64 out_stride, u64 n, hipStream_t stream);

// merkle.hip
int merkle_inner_launch(u64* d_nodes, u32 depth, u64 n_leaves, hipStream_t stream, u64* root_out = nullptr, u64 seq = 0);
int merkle_build_xfe_launch(const u64* d_limbs, u64 limb_stride, u64 n, u64* d_nodes, hipStream_t stream, u64* root_out = nullptr, u64 seq = 0);
int merkle_build_bfe_launch(const u64* d_values, u64 n, u64* d_nodes, hipStream_t stream);
int merkle_build_bytes_launch(const u64* d_data, const u64* d_offsets, const u32* d_lengths, u64 n, u64* d_nodes, hipStream_t stream);

// coset.hip: the tree with one leaf per folding coset
int coset_tree_launch(const FriFoldArgs* fold, u64* d_cw, u64 cw_stride, u64 q, u32 log2_coset, u64* d_nodes, hipStream_t stream, u64* not_mine,
                      u64 token, u64* root_out, u64 seq);
int coset_tree_rows(const u64* d_cw, u64 cw_stride, u64 q, u32 log2_coset, u64* d_nodes, unsigned char h_root[64], hipStream_t stream);

// pow.hip: the smallest nonce in [first, first + count) whose hash with `seed` starts with `bits` zero bits (pow_core.hpp); bounded
// launches in ascending order, the stream synchronised after each.  POW_DEFAULT_WINDOW: the nonces of one search step of a FRI
// session that was given no window of its own -- one full launch, a millisecond or two.
constexpr u64 POW_DEFAULT_WINDOW = 1ULL << 24;
int pow_search(const u64 seed[4], u32 bits, u64 first, u64 count, u64* nonce, bool* found, hipStream_t stream);

// pinned, device-visible staging for one gather call: a lease on a block of the pooled pinned-host allocator (runtime.cpp:
// mutex-guarded, size classes, no hipHostMalloc / hipHostFree on the hot path).  One lease per call, so that concurrent provers
// -- threads, or several devices driven by one process -- never share a staging buffer; the lease goes back when the call returns.
struct PinnedLease {
    void* host = nullptr;
    void* dev = nullptr;
    int get(size_t need) {
        BFS_TRY(host_alloc(need < 4096 ? 4096 : need, &host));
        BFS_HIP(hipHostGetDevicePointer(&dev, host, 0));
        return BFS_OK;
    }
    ~PinnedLease() { if (host) (void)host_release(host); }
    PinnedLease() = default;
    PinnedLease(const PinnedLease&) = delete;
    PinnedLease& operator=(const PinnedLease&) = delete;
};

}  // namespace bfs
