// coset.hip -- Merkle trees with one leaf per FRI folding coset (Fri(..., coset_leaves=True)): leaf c of a codeword C of length a * q is
//     blake2b(pickle.dumps((C[c], C[c + q], .., C[c + (a - 1) q]))),   a = 2, 4 or 8,
// the reference's Merkle over a list of tuples (/root/reference/code/merkle.py:8-41).  One kernel serves round 0 (the codeword is in
// HBM) and the later rounds (every thread first PRODUCES its a elements with the fold of the previous round, fri.py:127-128, and
// stores them for the openings); the levels above the leaves are merkle.hip's, unchanged.
#include <atomic>
#include <vector>

#include "../../include/bfstark.h"
#include "coset_core.hpp"
#include "runtime.hpp"

namespace bfs {

constexpr u32 COSET_THREADS = 64;     // one wavefront per workgroup: 16.5 KiB of LDS, nine workgroups per CU

// Thread c < q: leaf c.  K > 0: cw does not exist yet -- element c + m q of it is fri_fold_point<K>(f, c + m q), written to cw on the way
// (f.half = A q); K = 0: cw is read.  Pass 1 makes (or reads) the A elements one at a time, because the length of the pickle -- the
// frame header, in block 0 -- depends on how long all 3 A integers are; pass 2 takes the elements back from cw one stage ahead of
// where they are written (the thread's own stores: L1 / L2 hits), so that no more than two elements are ever held in registers.
// not_mine: a tuple with an element whose top limb is zero is not hashed; *not_mine = token tells the host (see coset_core.hpp).
template <int K, int A>
__global__ void __launch_bounds__(COSET_THREADS) coset_leaves_kernel(FriFoldArgs f, u64* cw, u64 cw_stride, u64 q, u64* leaf_digests,
                                                                     const u64* block0_states, u64* not_mine, u64 token) {
    typedef CosetShape<A> Shape;
    __shared__ __attribute__((aligned(16))) unsigned char blk[COSET_LANE_BYTES * COSET_THREADS];
    unsigned char* const buf = blk + COSET_LANE_BYTES * threadIdx.x;
    const u64 c = (u64)blockIdx.x * COSET_THREADS + threadIdx.x;
    bool ok = c < q;
    u32 int_bytes = 0;
    if (ok) {
#pragma nounroll
        for (u32 m = 0; m < (u32)A; ++m) {
            const u64 at = c + (u64)m * q;
            u64 c0, c1, c2;
            if constexpr (K > 0) {
                const Xfe r = fri_fold_point<K>(f, at);
                c0 = r.c[0]; c1 = r.c[1]; c2 = r.c[2];
                cw[at] = c0; cw[cw_stride + at] = c1; cw[2 * cw_stride + at] = c2;
            } else {
                c0 = cw[at]; c1 = cw[cw_stride + at]; c2 = cw[2 * cw_stride + at];
            }
            int_bytes += pickle_int_len(c0) + pickle_int_len(c1) + pickle_int_len(c2);
            ok = ok && c2 != 0;
        }
        if (!ok) __hip_atomic_store(not_mine, token, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    CosetLane s;
    s.pos = 0; s.consumed = 128; s.total = Shape::CONST_BYTES + int_bytes;
    u64 x0 = 0, x1 = 0, x2 = 0;                       // the element of the coming stage
    if (ok) {
        const u64* ms = block0_states + (size_t)(int_bytes - Shape::MIN_INT_BYTES) * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) s.h[j] = ms[j];
        x0 = cw[c]; x1 = cw[cw_stride + c]; x2 = cw[2 * cw_stride + c];
    }
    u32 stage = 0;
    bool done = false;
    while (true) {
        stage = (u32)__builtin_amdgcn_readfirstlane(stage);      // (the same in every lane; the compiler cannot tell)
        // ---- the compression site
        const bool behind = __any(ok && s.pos < 128);          // (voted by the whole wave, in front of the lane's own conditions)
        bool want;
        if (!done) want = ok && coset_lane_ready(s) && (s.pos > COSET_FORCE || !behind);
        else want = ok && s.consumed < s.total;
        if (__any(want)) {
            if (want) coset_compress(s, buf, done);
            continue;
        }
        if (done) break;
        if (ok) {
            coset_stage<A>(s, buf, stage, x0, x1, x2);
            if (stage >= 2 && stage + 1 < Shape::STAGES) {         // stage + 1 writes element stage - 1
                const u64 at = c + (u64)(stage - 1) * q;
                x0 = cw[at]; x1 = cw[cw_stride + at]; x2 = cw[2 * cw_stride + at];
            }
        }
        ++stage;
        done = stage == Shape::STAGES;
    }
    if (!ok) return;
    u64* out = leaf_digests + c * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = s.h[j];
}

template <int A>
static int coset_block0_states(const u64** d_table) {
    constexpr u64 KEY = 0x636F736574ULL;      // "coset"
    if (cached_table_lookup(KEY, A, 0, d_table)) return BFS_OK;
    std::vector<u64> host((size_t)CosetShape<A>::BLOCK0_STATES * 8);
    for (u32 e = 0; e < CosetShape<A>::BLOCK0_STATES; ++e) {
        unsigned char block[128];
        coset_block0<A>(CosetShape<A>::MIN_INT_BYTES + e, block);
        u64 m[16], st[8];
        memcpy(m, block, 128);
        blake2b_init(st);
        blake2b_compress(st, m, 128, false);
        memcpy(&host[(size_t)e * 8], st, 64);
    }
    return cached_table(KEY, A, 0, host.data(), host.size(), d_table);
}

template <int KF, int A = 1 << KF>
static int coset_leaves_launch_a(const FriFoldArgs* fold, u64* d_cw, u64 cw_stride, u64 q, u64* d_leaf_digests, hipStream_t stream, u64* not_mine, u64 token) {
    const u64* d_states = nullptr;
    BFS_TRY(coset_block0_states<A>(&d_states));
    const dim3 grid((u32)((q + COSET_THREADS - 1) / COSET_THREADS)), block(COSET_THREADS);
    if (fold != nullptr) hipLaunchKernelGGL((coset_leaves_kernel<KF, A>), grid, block, 0, stream, *fold, d_cw, cw_stride, q, d_leaf_digests, d_states, not_mine, token);
    else hipLaunchKernelGGL((coset_leaves_kernel<0, A>), grid, block, 0, stream, FriFoldArgs{}, d_cw, cw_stride, q, d_leaf_digests, d_states, not_mine, token);
    BFS_HIP(hipGetLastError());
    return BFS_OK;
}

// The coset tree of a codeword of a * q elements, a = 2^log2_coset: q leaf digests at d_nodes + 8 q words, the levels above them, the root
// through the mailbox when root_out is given.  fold != NULL: the codeword is the fold of the previous round's (fold->half = a q, fold by
// a) and is written to d_cw.  *not_mine (pinned, device-visible) = token afterwards: some tuple was left to coset_tree_rows.
int coset_tree_launch(const FriFoldArgs* fold, u64* d_cw, u64 cw_stride, u64 q, u32 log2_coset, u64* d_nodes, hipStream_t stream, u64* not_mine,
                      u64 token, u64* root_out, u64 seq) {
    if (q == 0 || (q & (q - 1))) { set_error("internal: coset tree over %llu leaves", (unsigned long long)q); return BFS_ERR_BAD_ARG; }
    if (fold != nullptr && (fold->log2_folding != log2_coset || fold->half != (q << log2_coset))) { set_error("internal: coset tree and fold disagree"); return BFS_ERR_BAD_ARG; }
    BFS_TRY(with_fold_factor(log2_coset, [&](auto k) -> int {
        return coset_leaves_launch_a<decltype(k)::value>(fold, d_cw, cw_stride, q, d_nodes + q * 8, stream, not_mine, token);
    }));
    return merkle_inner_launch(d_nodes, tree_depth(q), q, stream, root_out, seq);
}

static std::atomic<u64> g_coset_trees_by_rows{0};     // how often a coset tree went through the interpreter (the tests ask)

// the same tree by the zipped-row interpreter: a columns that are slices of the codeword, q apart, unsalted.  Every pattern of stored
// coefficients; synchronises the stream.
int coset_tree_rows(const u64* d_cw, u64 cw_stride, u64 q, u32 log2_coset, u64* d_nodes, unsigned char h_root[64], hipStream_t stream) {
    bfs_row_column cols[8];
    const u32 a = 1u << log2_coset;
    g_coset_trees_by_rows.fetch_add(1, std::memory_order_relaxed);
    for (u32 m = 0; m < a; ++m) cols[m] = bfs_row_column{d_cw + (u64)m * q, 1, 0};
    return bfs_merkle_build_rows_root(cols, a, q, cw_stride, nullptr, 0, (uint8_t*)d_nodes, h_root, stream);
}

}  // namespace bfs

using namespace bfs;

extern "C" uint64_t bfs_coset_trees_by_rows(void) { return g_coset_trees_by_rows.load(std::memory_order_relaxed); }

extern "C" int bfs_merkle_build_xfe_cosets(const uint64_t* d_limbs, uint64_t limb_stride, uint64_t n, uint32_t log2_coset, uint8_t* d_nodes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (((uintptr_t)d_nodes & 15) != 0) { set_error("d_nodes must be 16-byte aligned"); return BFS_ERR_BAD_ARG; }
    if (log2_coset < 1 || log2_coset > 3) { set_error("bfs_merkle_build_xfe_cosets: log2_coset must be 1, 2 or 3 (got %u)", log2_coset); return BFS_ERR_BAD_ARG; }
    if (n == 0 || (n & (n - 1)) || (n >> log2_coset) == 0) { set_error("bfs_merkle_build_xfe_cosets: n must be a power of two, at least the coset size"); return BFS_ERR_BAD_ARG; }
    if (limb_stride < n) { set_error("bfs_merkle_build_xfe_cosets: limb_stride < n"); return BFS_ERR_BAD_ARG; }
    PinnedLease flag;
    BFS_TRY(flag.get(64));
    volatile u64* seen = (volatile u64*)flag.host;
    *seen = 0;
    const u64 q = n >> log2_coset;
    BFS_TRY(coset_tree_launch(nullptr, (u64*)d_limbs, limb_stride, q, log2_coset, (u64*)d_nodes, stream, (u64*)flag.dev, 1, nullptr, 0));
    BFS_HIP(hipStreamSynchronize(stream));
    if (*seen == 0) return BFS_OK;
    return coset_tree_rows(d_limbs, limb_stride, q, log2_coset, (u64*)d_nodes, nullptr, stream);
}
