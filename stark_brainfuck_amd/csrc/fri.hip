// fri.hip -- the FRI prover loop on gfx950.  Replaces Fri.commit / Fri.query / Fri.query_last / Fri.prove of the
// reference (/root/reference/code/fri.py:91-199): per round a Merkle tree over the codeword (GPU), the root to the
// host, the Fiat-Shamir challenge from the transcript (host: pickle + SHAKE256, ip.py:21-22), the split-and-fold
// step (GPU, fri.py:127-128); then index sampling (fri.py:62-86) and one batched gather of every revealed leaf and
// authentication-path node.
// Both halves plan first and run second.  fri_commit: plan_rounds checks the arguments, lays every round out in one block and names
// the kernels of its tree (TreePath); the round loop is launch_round_tree, await_root, the transcript step, the next fold's constants.
// fri_query: one list of openings in the reference's push order (Opening) gives the gather requests and, after the one gather
// (gather_run, shared with the STARK openings and bfs_gather), the tuples and paths that are pushed.
#include <algorithm>
#include <chrono>
#include <map>
#include <unordered_map>
#include <vector>

#include "../../include/bfstark.h"
#include "blake2b.hpp"
#include "refpickle.hpp"
#include "runtime.hpp"

namespace bfs {

// the fold on its own (fri.py:127-128, K times: fri_fold_point in runtime.hpp): out[i], i < f.half, from the 2^K inputs in[i + m * f.half]
// winv_*: two-level powers of the ROUND-0 omega^-1 (exponent i << round_shift)
// (launched with 256 threads; saying so gives the K = 3 body, which holds 8 extension elements, the registers it needs: without the
//  bound the compiler keeps to 128 VGPRs and spills two.  K = 1 keeps the default bound and with it the code it had.)
template <int K>
__global__ void __launch_bounds__(K == 1 ? 1024 : 256) fri_fold_kernel(FriFoldArgs f, u64* out, u64 out_stride) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < f.half; i += (u64)gridDim.x * blockDim.x) {
        const Xfe r = fri_fold_point<K>(f, i);
        out[i] = r.c[0];
        out[out_stride + i] = r.c[1];
        out[2 * out_stride + i] = r.c[2];
    }
}

constexpr u32 FRI_FOLD_GRID_MAX = 4096;       // workgroups of 256; longer codewords go round the grid-stride loop
static int fri_fold_launch(const FriFoldArgs& f, u64* out, u64 out_stride, hipStream_t stream) {
    u32 grid = (u32)((f.half + 255) / 256);
    if (grid > FRI_FOLD_GRID_MAX) grid = FRI_FOLD_GRID_MAX;
    return with_fold_factor(f.log2_folding, [&](auto k) -> int {
        hipLaunchKernelGGL(fri_fold_kernel<decltype(k)::value>, dim3(grid), dim3(256), 0, stream, f, out, out_stride);
        BFS_HIP(hipGetLastError());
        return BFS_OK;
    });
}

// one request = `nwords` 64-bit words at base, base + stride, ...; requests and results live in pinned host memory that the
// GPU reads / writes directly (no copy commands: the openings of a proof are a few thousand scattered words)
struct GatherReq {
    const u64* base;
    u32 nwords, stride;
    u64 out_offset;
};
__global__ void gather_requests_kernel(const GatherReq* req, u32 count, u64* out) {
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
        const GatherReq r = req[i];
        for (u32 w = 0; w < r.nwords; ++w) out[r.out_offset + w] = r.base[(u64)w * r.stride];
    }
}

// the gather sequence: the requests into a pinned area the GPU reads, one launch, the stream synchronised; *words = the `nwords` gathered
// words, in a pinned area the GPU wrote (valid while the caller holds the two leases).  reqs is not empty.
static int gather_run(const std::vector<GatherReq>& reqs, u64 nwords, hipStream_t stream, PinnedLease& req_area, PinnedLease& res_area, const u64** words) {
    BFS_TRY(req_area.get(reqs.size() * sizeof(GatherReq)));
    BFS_TRY(res_area.get(nwords * sizeof(u64)));
    memcpy(req_area.host, reqs.data(), reqs.size() * sizeof(GatherReq));
    hipLaunchKernelGGL(gather_requests_kernel, dim3((u32)((reqs.size() + 255) / 256)), dim3(256), 0, stream, (const GatherReq*)req_area.dev, (u32)reqs.size(),
                       (u64*)res_area.dev);
    BFS_HIP(hipGetLastError());
    BFS_HIP(hipStreamSynchronize(stream));
    *words = (const u64*)res_area.host;
    return BFS_OK;
}

// wall-clock breakdown of the last bfs_fri_commit / bfs_fri_query on this thread (ms): see bfs_fri_last_timing
static thread_local double g_fri_timing[8] = {0, 0, 0, 0, 0, 0, 0, 0};
static inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Which kernels build a round's tree.  plan_rounds decides it from the round's length and position; launch_round_tree acts on it.
enum class TreePath : unsigned char {
    Borrowed,       // round 0: the tree the caller has built over the input codeword (bfs_fri_session_round0_tree / _round0_coset_tree)
    Coset,          // one leaf per folding coset (coset.hip); the leaf kernel makes the codeword on the way in rounds >= 1
    OneLaunch,      // length <= FRI_FUSED_MAX: fold + leaves + subtrees in one launch (fri_round_quad_kernel)
    FoldInLeaves,   // a longer round >= 1: the leaf kernel folds the previous round's codeword on the way
    Codeword,       // a longer round 0: the tree over the codeword that is there (fri.py:108)
    SingleElement,  // length 1: fold on its own, the leaf is the root, copied back without the mailbox
};

struct FriRound {
    const u64* cw = nullptr;  // limb-major codeword
    u64 stride = 0, length = 0;
    u64 leaves = 0;           // leaves of the round's tree: length, or length / a when the round commits one leaf per coset
    u64* nodes = nullptr;     // 2*leaves digests of 8 words
    TreePath path = TreePath::Codeword;
    unsigned char root[64];
};

// pinned, host-visible mailbox the tree kernel drops each round's root into: words 0-7 the digest, word 8 the sequence flag; word 9 is
// the coset-leaf kernel's not_mine token (coset.hip)
struct RootMailbox {
    u64* host = nullptr;
    u64* dev = nullptr;
    u64 seq = 0;
    int init() {
        if (host) return BFS_OK;
        BFS_TRY(host_alloc(16 * sizeof(u64), (void**)&host));       // pooled: hipHostFree per session stalls later dispatches
        memset(host, 0, 16 * sizeof(u64));
        BFS_HIP(hipHostGetDevicePointer((void**)&dev, host, 0));
        return BFS_OK;
    }
    ~RootMailbox() { if (host) (void)host_release(host); }
};

struct FriSession {
    std::vector<FriRound> rounds;
    void* block = nullptr;  // device allocation owned by the session (null when it borrows the cached workspace)
    bool use_workspace = false;
    RootMailbox mailbox;
    u32 log_n = 0;
    u32 log2_folding = 1;   // every round folds its codeword by 2^log2_folding (bfs_fri_session_set_folding)
    bool coset_leaves = false;   // every round but the last commits one leaf per folding coset (bfs_fri_session_set_coset_leaves)
    u32 grinding_bits = 0;       // bfs_fri_query grinds a nonce of that many zero bits before it draws the indices (bfs_fri_session_set_grinding)
    u64 grinding_window = POW_DEFAULT_WINDOW;   // nonces per search step
    u64 round0_leaves = 0;       // leaves of round0_nodes' tree when the caller said (bfs_fri_session_round0_coset_tree), else 0
    // (round, index) -> the element / tree-node object.  One object per key: the reference pushes the same Python object
    // again when an index recurs, and pickle memoises by identity.
    struct Key {
        u64 v;
        Key(u32 round, u64 index) : v(((u64)round << 48) | index) {}
        bool operator==(const Key& o) const { return v == o.v; }
    };
    // open-addressing table (linear probing, power-of-two capacity): a proof makes ~4 000 look-ups and insertions here, and
    // std::unordered_map's node allocations were 0.2 ms of a 1.9 ms proof
    struct KeyMap {
        std::vector<u64> keys;          // key.v + 1; 0 = empty slot
        std::vector<u32> slots;         // index into vals
        std::vector<rp::Ref> vals;      // in insertion order
        void reserve(size_t n) { size_t cap = 64; while (cap < 2 * n) cap <<= 1; if (cap > keys.size()) rehash(cap); vals.reserve(n); }
        void rehash(size_t cap) {
            std::vector<u64> k2(cap, 0);
            std::vector<u32> s2(cap, 0);
            for (size_t i = 0; i < keys.size(); ++i)
                if (keys[i]) { size_t j = slot_of(keys[i], cap); while (k2[j]) j = (j + 1) & (cap - 1); k2[j] = keys[i]; s2[j] = slots[i]; }
            keys.swap(k2); slots.swap(s2);
        }
        static size_t slot_of(u64 stored, size_t cap) { return (size_t)((stored * 0x9E3779B97F4A7C15ULL) >> 20) & (cap - 1); }
        // the slot of `key`: existing, or the empty one where it goes
        size_t find(const Key& key) const {
            size_t j = slot_of(key.v + 1, keys.size());
            while (keys[j] && keys[j] != key.v + 1) j = (j + 1) & (keys.size() - 1);
            return j;
        }
        bool count(const Key& key) const { return !keys.empty() && keys[find(key)] != 0; }
        rp::Ref& operator[](const Key& key) {
            if (2 * (vals.size() + 1) > keys.size()) rehash(keys.empty() ? 64 : 2 * keys.size());
            const size_t j = find(key);
            if (!keys[j]) { keys[j] = key.v + 1; slots[j] = (u32)vals.size(); vals.emplace_back(); }
            return vals[slots[j]];
        }
    };
    KeyMap elements, nodes;
    std::vector<uint64_t> last_handles;
    hipStream_t block_stream = nullptr;
    const u64* round0_nodes = nullptr;     // a tree over the input codeword that the caller has already built (bfs_fri_session_round0_tree)
    unsigned char round0_root[64];
    ~FriSession() { if (block) (void)device_release(block, block_stream); }
};

// Every round is at least 2 long when expansion >= 1: with h halvings, N >> h <= expansion < N >> (h - 1), and the last of the
// R = (h - 1) / k + 1 rounds has length N >> k (R - 1) >= N >> (h - 1) > expansion >= 1.  Only expansion = 0 (h = log2 N + 1) ends on a
// single element, when k divides log2 N: TreePath::SingleElement.
static u32 fri_num_rounds(u64 length, u32 expansion, u32 k = 1) {  // fri.py:54-60; folding by 2^k: floor((that - 1) / k) folds, one codeword more
    u32 r = 0;
    while (length > expansion) { length /= 2; ++r; }
    return r == 0 ? 0 : (r - 1) / k + 1;
}

// (N, expansion, k, coset leaves, round-0 tree) -> S.rounds: the argument checks, one allocation for the nodes of every round and the
// codewords of rounds >= 1, and per round its length, leaves, place in the block and tree path
static int plan_rounds(FriSession& S, const u64* d_cw, u64 stride, u32 log_n, u64 omega, u32 expansion, hipStream_t stream) {
    const u64 N = 1ull << log_n;
    const u32 k = S.log2_folding;
    const u32 R = fri_num_rounds(N, expansion, k);
    if (k > 1 && R < 2) { set_error("cannot fold by %u with less than one fold", 1u << k); return BFS_ERR_BAD_ARG; }
    if (R < 1) { set_error("cannot do FRI with less than one round"); return BFS_ERR_BAD_ARG; }
    if (gl_pow(omega, N) != 1 || (log_n && gl_pow(omega, N / 2) == 1)) {
        set_error("error in commit: omega does not have the right order!");
        return BFS_ERR_NOT_ROOT;
    }
    S.log_n = log_n;
    S.rounds.assign(R, FriRound());
    const bool coset = S.coset_leaves;
    if (coset && R < 2) { set_error("cannot commit to cosets with less than one fold"); return BFS_ERR_BAD_ARG; }
    if (S.round0_nodes && S.round0_leaves != (coset ? N >> k : 0)) {
        set_error("the round-0 tree handed to the session has %llu leaves, this session's has %llu", (unsigned long long)(S.round0_leaves ? S.round0_leaves : N),
                  (unsigned long long)(coset ? N >> k : N));
        return BFS_ERR_BAD_ARG;
    }
    size_t words = 0;
    for (u32 r = 0; r < R; ++r) {
        FriRound& fr = S.rounds[r];
        const bool coset_round = coset && r + 1 < R;
        fr.length = N >> (k * r);
        fr.leaves = coset_round ? fr.length >> k : fr.length;
        fr.path = r == 0 && S.round0_nodes ? TreePath::Borrowed
                  : coset_round            ? TreePath::Coset
                  : fr.length < 2          ? TreePath::SingleElement
                  : fr.length <= FRI_FUSED_MAX ? TreePath::OneLaunch
                  : r >= 1                 ? TreePath::FoldInLeaves
                                           : TreePath::Codeword;
        words += (size_t)16 * fr.leaves + (r ? (size_t)3 * fr.length : 0);
    }
    u64* p = nullptr;
    if (S.use_workspace) {
        void* w = nullptr;
        BFS_TRY(workspace(4, words * sizeof(u64), stream, &w));   // bfs_fri_prove: nothing outlives the call
        p = (u64*)w;
    } else {
        if (S.block) { (void)device_release(S.block, S.block_stream); S.block = nullptr; }
        BFS_TRY(device_alloc(words * sizeof(u64), stream, &S.block));
        S.block_stream = stream;
        p = (u64*)S.block;
    }
    for (u32 r = 0; r < R; ++r) {
        FriRound& fr = S.rounds[r];
        fr.nodes = p; p += 16 * fr.leaves;
        if (r == 0) { fr.cw = d_cw; fr.stride = stride; }
        else { fr.cw = p; fr.stride = fr.length; p += 3 * fr.length; }
    }
    return S.mailbox.init();
}

// The kernels of round r's tree.  fold: what makes the round's codeword out of the previous one's (fold.in == nullptr in round 0, whose
// codeword is there); every path of a round >= 1 folds on the way.  *seq != 0 afterwards: the root comes through the mailbox under that
// sequence number (await_root); 0: fr.root is set (Borrowed) or the caller copies it back (SingleElement).
static int launch_round_tree(FriSession& S, u32 r, const FriFoldArgs& fold, hipStream_t stream, u64* seq) {
    FriRound& fr = S.rounds[r];
    const bool folds = fold.in != nullptr;
    u64* const cw = (u64*)fr.cw;
    u64* const box = S.mailbox.dev;
    *seq = 0;
    if (folds != (r >= 1)) { set_error("internal: round %u of the plan and its fold disagree", r); return BFS_ERR_BAD_ARG; }
    switch (fr.path) {
    case TreePath::Borrowed:
        fr.nodes = (u64*)S.round0_nodes;          // the STARK prover has just committed to this very codeword (brainfuck_stark.py:301 / fri.py:108)
        memcpy(fr.root, S.round0_root, 64);
        return BFS_OK;
    case TreePath::SingleElement:
        if (folds) BFS_TRY(fri_fold_launch(fold, cw, fr.stride, stream));
        return merkle_build_xfe_launch(fr.cw, fr.stride, fr.length, fr.nodes, stream);
    case TreePath::Coset:
        // the levels above the fr.leaves leaves and the root's way to the host are those of the per-element tree
        *seq = ++S.mailbox.seq;
        return coset_tree_launch(folds ? &fold : nullptr, cw, fr.stride, fr.leaves, S.log2_folding, fr.nodes, stream, box + 9, *seq, box, *seq);
    case TreePath::OneLaunch:
        *seq = ++S.mailbox.seq;
        return fri_round_fused_launch(fold, cw, fr.stride, fr.length, fr.nodes, stream, box, *seq);
    case TreePath::FoldInLeaves:
        *seq = ++S.mailbox.seq;
        return merkle_build_xfe_fold_launch(fold, cw, fr.stride, fr.length, fr.nodes, stream, box, *seq);
    case TreePath::Codeword:
        *seq = ++S.mailbox.seq;
        return merkle_build_xfe_launch(fr.cw, fr.stride, fr.length, fr.nodes, stream, box, *seq);  // fri.py:108
    }
    set_error("internal: round %u has no tree path", r);
    return BFS_ERR_BAD_ARG;
}

int fri_commit(FriSession& S, rp::Transcript& ps, const u64* d_cw, u64 stride, u32 log_n, u64 offset, u64 omega,
               u32 expansion, hipStream_t stream) {
    const double t_begin = now_ms();
    BFS_TRY(plan_rounds(S, d_cw, stride, log_n, omega, expansion, stream));
    const u32 k = S.log2_folding;
    const u32 R = (u32)S.rounds.size();
    const u64 *winv_lo = nullptr, *winv_hi = nullptr;
    u32 lo_bits = 0;
    BFS_TRY(ntt_power_tables(gl_inv(omega), log_n, &winv_lo, &winv_hi, &lo_bits));
    u64 g = offset, w = omega;                     // offset and generator of round r's domain
    FriFoldArgs fold{};                            // the fold that produces round r's codeword; none in round 0
    // Fiat-Shamir look-ahead: with a long transcript in front (a STARK proof: tens of KB), helper threads absorb the SHAKE256 prefix of
    // every coming challenge now (Transcript::Lookahead); rounds 1 .. R-2 push a root and draw a challenge
    rp::Transcript::Lookahead look;
    static const bool lookahead_on = getenv("BFS_FRI_LOOKAHEAD") == nullptr || atoi(getenv("BFS_FRI_LOOKAHEAD")) != 0;
    static const bool trace = getenv("BFS_FRI_TRACE") != nullptr;      // development aid: host timeline of every round on stderr
    // (begun behind round 1's launch, below: laying out the R - 2 pickles takes ~50 us with a STARK proof's openings in front, and
    //  nothing is pushed before round 1's root -- so the GPU hashes round 1 meanwhile instead of waiting for it)
    bool looking = false, look_begun = false;
    auto begin_lookahead = [&]() {
        if (look_begun) return;
        look_begun = true;
        const double t_look = trace ? now_ms() : 0;
        looking = lookahead_on && R >= 3 && ps.lookahead_begin(look, R - 2);
        if (trace) fprintf(stderr, "fri look-ahead %s: %.1f us, %zu objects in front\n", looking ? "on" : "off", 1e3 * (now_ms() - t_look), ps.objects.size());
    };
    for (u32 r = 0; r < R; ++r) {
        FriRound& fr = S.rounds[r];
        unsigned char seed[32];
        bool have_seed = false, speculating = false;
        const double t_round = trace ? now_ms() : 0;
        double t_launched = 0, t_absorbed = 0, t_root = 0;
        rp::Transcript::Speculation speculation;
        // what follows every launch of a tree whose root comes through the mailbox.  The tree kernel writes the root straight into pinned
        // host memory; poll the sequence flag instead of paying a copy command + stream synchronisation per round.  While the GPU
        // hashes: the next challenge is SHAKE256 of the WHOLE transcript including this root (fri.py:112-120), tens of KB -- as long as
        // the tree kernels of the late rounds.  Everything in front of the root's 64 bytes is known already, so the sponge absorbs it
        // now and only the last block or two wait for the root.
        auto await_root = [&](u64 seq) -> int {
            if (trace) t_launched = now_ms();
            if (r >= 1) begin_lookahead();
            if (r + 1 < R) {
                if (r == 0) { ps.fiat_shamir(ps.objects.size(), seed, 32); have_seed = true; }
                else if (!looking) { ps.speculate(speculation); speculating = true; }
            }
            if (trace) t_absorbed = now_ms();
            volatile u64* flag = S.mailbox.host + 8;
            u64 spins = 0;
            while (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq) {
                if (++spins > (1ull << 22)) {   // ~ms: fall back to a real synchronisation (also surfaces kernel errors)
                    BFS_HIP(hipStreamSynchronize(stream));
                    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq) { set_error("root mailbox was not written"); return BFS_ERR_HIP; }
                    break;
                }
            }
            memcpy(fr.root, S.mailbox.host, 64);
            return BFS_OK;
        };
        u64 seq = 0;
        BFS_TRY(launch_round_tree(S, r, fold, stream, &seq));
        if (seq != 0) {
            BFS_TRY(await_root(seq));
            if (fr.path == TreePath::Coset && __atomic_load_n(S.mailbox.host + 9, __ATOMIC_ACQUIRE) == seq) {
                // a tuple with an element that stores fewer than three coefficients: the zipped-row interpreter hashes the tree again
                // (the codeword is in HBM by now) -- every other codeword than one lifted from the base field never comes here
                BFS_TRY(coset_tree_rows(fr.cw, fr.stride, fr.leaves, k, fr.nodes, fr.root, stream));
            }
        } else if (fr.path == TreePath::SingleElement) {
            if (r >= 1) begin_lookahead();
            BFS_HIP(hipMemcpyAsync(fr.root, fr.nodes + 8, 64, hipMemcpyDeviceToHost, stream));
            BFS_HIP(hipStreamSynchronize(stream));
        }
        if (trace) t_root = now_ms();
        if (speculating) ps.resolve(speculation, fr.root, seed, 32);          // the placeholder pushed by speculate() becomes the root
        else if (r > 0 && looking) { ps.lookahead_next(look, fr.root, r + 1 < R ? seed : nullptr, 32); have_seed = r + 1 < R; }
        else if (r > 0) ps.objects.push_back(rp::mk_bytes(fr.root, 64));      // fri.py:112-113
        if (trace)
            fprintf(stderr, "fri round %2u  n %8llu  launch %6.1f us  absorb %6.1f us  wait %6.1f us  finish %6.1f us\n", r, (unsigned long long)fr.length,
                    1e3 * (t_launched - t_round), 1e3 * (t_absorbed - t_launched), 1e3 * (t_root - t_absorbed), 1e3 * (now_ms() - t_root));
        if (r == R - 1) break;                                                // fri.py:116-117
        if (!speculating && !have_seed) ps.fiat_shamir(ps.objects.size(), seed, 32);   // fri.py:120
        // the next round folds while it builds its tree
        fold.in = fr.cw; fold.in_stride = fr.stride;
        fold.winv_lo = winv_lo; fold.winv_hi = winv_hi; fold.lo_bits = lo_bits; fold.round_shift = k * r;
        fri_fold_constants(fold, k, fr.length, rp::sample_xfe(seed, 32), g, w);
        for (u32 j = 0; j < k; ++j) { g = gl_sqr(g); w = gl_sqr(w); }  // fri.py:130-131, once per step (the kernels square omega through round_shift)
    }
    g_fri_timing[0] = now_ms() - t_begin;   // rounds: trees, roots, challenges, folds
    // fri.py:134: the last codeword goes into the transcript as a list of element objects
    FriRound& last = S.rounds[R - 1];
    std::vector<u64> host(3 * last.length);
    if (last.stride == last.length) {
        BFS_HIP(hipMemcpyAsync(host.data(), last.cw, 3 * last.length * sizeof(u64), hipMemcpyDeviceToHost, stream));
    } else {
        for (int k = 0; k < 3; ++k)
            BFS_HIP(hipMemcpyAsync(host.data() + k * last.length, last.cw + k * last.stride, last.length * sizeof(u64), hipMemcpyDeviceToHost, stream));
    }
    BFS_HIP(hipStreamSynchronize(stream));
    std::vector<rp::Ref> items;
    for (u64 j = 0; j < last.length; ++j) {
        u64 l[3] = {host[j], host[last.length + j], host[2 * last.length + j]};
        rp::Ref e = ps.world.xfe_compact(l);
        S.elements[FriSession::Key(R - 1, j)] = e;
        items.push_back(e);
    }
    ps.objects.push_back(rp::mk_list(items));
    g_fri_timing[1] = now_ms() - t_begin - g_fri_timing[0];   // last codeword to the host
    return BFS_OK;
}

// fri.py:62-86
static int sample_indices(const unsigned char seed[32], u64 size, u64 reduced_size, u32 number, std::vector<u64>& out) {
    if (number > reduced_size) {
        set_error("cannot sample more indices than available in last codeword; requested: %u, available: %llu", number, (unsigned long long)reduced_size);
        return BFS_ERR_TOO_MANY_INDICES;
    }
    out.clear();
    std::vector<u64> reduced;
    std::vector<unsigned char> msg(seed, seed + 32);
    while (out.size() < number) {
        unsigned char digest[64];
        blake2b_host(msg.data(), msg.size(), digest);  // blake2b(seed + bytes(counter)): `counter` zero bytes
        msg.push_back(0);
        u128 acc = 0;
        for (int i = 0; i < 64; ++i) acc = ((acc << 8) | digest[i]) % size;
        u64 index = (u64)acc, red = index % reduced_size;
        bool seen = false;
        for (u64 x : reduced) seen |= (x == red);
        if (!seen) { out.push_back(index); reduced.push_back(red); }
    }
    return BFS_OK;
}

// proof of work: the smallest nonce whose hash with the seed drawn after the last codeword starts with S.grinding_bits zero bits goes
// into the transcript as a plain int.  The windows ascend, so the first one with a hit holds the smallest nonce there is; the search
// gives up after 2^(bits + 6) nonces (a seed without a hit among them has probability e^-64).
static int fri_grind(const FriSession& S, const unsigned char seed[32], hipStream_t stream, rp::Transcript& ps) {
    u64 words[4];
    memcpy(words, seed, 32);
    const u64 limit = 1ULL << (S.grinding_bits + 6);
    for (u64 first = 0; first < limit;) {
        const u64 count = limit - first < S.grinding_window ? limit - first : S.grinding_window;
        u64 nonce = 0;
        bool found = false;
        BFS_TRY(pow_search(words, S.grinding_bits, first, count, &nonce, &found, stream));
        if (found) { ps.objects.push_back(rp::mk_int(nonce)); return BFS_OK; }
        first += count;
    }
    set_error("bfs_fri_query: no nonce of %u grinding bits among the first 2^%u", S.grinding_bits, S.grinding_bits + 6);
    return BFS_ERR_BAD_ARG;
}

int fri_query(FriSession& S, rp::Transcript& ps, u32 t, u64* h_top, hipStream_t stream) {
    const u32 R = (u32)S.rounds.size();
    if (R < 2) { set_error("Fri.prove needs at least two rounds (fri.py:186 indexes codewords[1])"); return BFS_ERR_BAD_ARG; }
    const double t_begin = now_ms();
    unsigned char seed[32];
    ps.fiat_shamir(ps.objects.size(), seed, 32);
    if (S.grinding_bits) {
        BFS_TRY(fri_grind(S, seed, stream, ps));
        ps.fiat_shamir(ps.objects.size(), seed, 32);      // the indices come from the stream that holds the nonce
    }
    std::vector<u64> top;
    BFS_TRY(sample_indices(seed, S.rounds[1].length, S.rounds[R - 1].length, t, top));  // fri.py:186-187
    for (u32 s = 0; s < t; ++s) h_top[s] = top[s];

    g_fri_timing[2] = now_ms() - t_begin;   // Fiat-Shamir + index sampling
    typedef FriSession::Key Key;
    const u32 fan = 1u << S.log2_folding;         // elements of round i that one element of round i + 1 depends on
    const bool coset = S.coset_leaves;            // a test opens one leaf of fan elements and one path per layer, nothing of the next round
    {   // what the openings can touch at most: fan + 1 elements and authentication paths per colinearity check and layer
        size_t depth_sum = 0;
        for (u32 r = 0; r < R; ++r) depth_sum += 64 - (size_t)__builtin_clzll(S.rounds[r].length);
        S.elements.reserve(S.elements.vals.size() + (size_t)(fan + 1) * t * R + 8);
        S.nodes.reserve((size_t)(fan + 1) * t * depth_sum / 2 + 64);
    }
    // every opening, once, in the reference's push order (fri.py:147-156, 166-174): per layer the t tuples -- the fan elements of round i
    // and, unless a leaf is a whole coset, the one of round i + 1 they fold to -- then per test the authentication paths.  The gather
    // requests below and the pushes at the end both come from this list.  (R - 2 layers are query(), the last one query_last(): the
    // last codeword is in the proof, so nothing of it gets a path)
    struct Opening {
        enum Kind : u32 { Element, TupleEnd /* an element that closes its tuple */, Path } kind;
        u32 round;
        u64 index;
    };
    std::vector<Opening> plan;
    plan.reserve((size_t)2 * (fan + 1) * t * (R - 1));
    for (u32 i = 0; i + 1 < R; ++i) {
        const u64 q = S.rounds[i + 1].length;      // = len(round i) / folding factor
        for (u32 s = 0; s < t; ++s) {
            const u64 c = top[s] % q;
            for (u32 m = 0; m < fan; ++m) plan.push_back({Opening::Element, i, c + m * q});
            if (!coset) plan.push_back({Opening::Element, i + 1, c});
            plan.back().kind = Opening::TupleEnd;
        }
        for (u32 s = 0; s < t; ++s) {
            const u64 c = top[s] % q;
            if (coset) { plan.push_back({Opening::Path, i, c}); continue; }
            for (u32 m = 0; m < fan; ++m) plan.push_back({Opening::Path, i, c + m * q});
            if (i + 2 < R) plan.push_back({Opening::Path, i + 1, c});
        }
    }
    std::vector<GatherReq> reqs;                // what to fetch
    std::vector<std::pair<int, Key>> order;      // what the fetched words are: (0 = element | 1 = tree node, key)
    reqs.reserve(4096); order.reserve(4096);
    u64 nwords = 0;
    auto need_element = [&](u32 r, u64 j) {
        Key key(r, j);
        if (S.elements.count(key)) return;       // same Python object in the reference -> same node here
        S.elements[key] = rp::Ref();
        order.push_back({0, key});
        const FriRound& fr = S.rounds[r];
        reqs.push_back(GatherReq{fr.cw + j, 3u, (u32)fr.stride, nwords});
        nwords += 3;
    };
    auto need_path = [&](u32 r, u64 leaf) {      // merkle.py:46-52
        const FriRound& fr = S.rounds[r];
        for (u64 k = fr.leaves | leaf; k > 1; k >>= 1) {
            Key key(r, k ^ 1);
            if (S.nodes.count(key)) continue;
            S.nodes[key] = rp::Ref();
            order.push_back({1, key});
            reqs.push_back(GatherReq{fr.nodes + (k ^ 1) * 8, 8u, 1u, nwords});
            nwords += 8;
        }
    };
    for (const Opening& o : plan) {
        if (o.kind == Opening::Path) need_path(o.round, o.index);
        else need_element(o.round, o.index);
    }
    g_fri_timing[3] = now_ms() - t_begin - g_fri_timing[2];   // planning the openings
    const double t_gather = now_ms();
    const u64* words = nullptr;
    PinnedLease req_area, res_area;
    if (!reqs.empty()) BFS_TRY(gather_run(reqs, nwords, stream, req_area, res_area, &words));
    g_fri_timing[4] = now_ms() - t_gather;   // gather kernel + synchronisation
    const double t_build = now_ms();
    size_t pos = 0;
    for (auto& o : order) {
        if (o.first == 0) {
            u64 l[3] = {words[pos], words[pos + 1], words[pos + 2]};
            pos += 3;
            S.elements[o.second] = ps.world.xfe_compact(l);
        } else {
            S.nodes[o.second] = rp::mk_bytes(words + pos, 64);
            pos += 8;
        }
    }
    auto path_obj = [&](u32 r, u64 leaf) {
        std::vector<rp::Ref> items;
        items.reserve(64 - (size_t)__builtin_clzll(S.rounds[r].leaves));
        for (u64 k = S.rounds[r].leaves | leaf; k > 1; k >>= 1) items.push_back(S.nodes[Key(r, k ^ 1)]);
        return rp::mk_list(std::move(items));
    };
    // push in the reference's order: per layer, t leaf triples then the authentication paths (fri.py:147-156, 166-174)
    std::vector<rp::Ref> items;
    items.reserve(fan + 1);
    for (const Opening& o : plan) {
        if (o.kind == Opening::Path) { ps.objects.push_back(path_obj(o.round, o.index)); continue; }
        items.push_back(S.elements[Key(o.round, o.index)]);
        if (o.kind == Opening::TupleEnd) { ps.objects.push_back(rp::mk_tuple(items)); items.clear(); }
    }
    g_fri_timing[5] = now_ms() - t_build;   // building the transcript objects
    return BFS_OK;
}

}  // namespace bfs

using namespace bfs;

extern "C" {

void* bfs_fri_session_new(void) { return new FriSession(); }
void bfs_fri_session_free(void* s) { delete (FriSession*)s; }

int bfs_fri_commit(void* session, void* ps, const uint64_t* d_codeword, uint64_t limb_stride, uint32_t log_n, uint64_t offset,
                   uint64_t omega, uint32_t expansion_factor, void* stream) {
    return fri_commit(*(FriSession*)session, *(rp::Transcript*)ps, d_codeword, limb_stride, log_n, offset, omega, expansion_factor, (hipStream_t)stream);
}

int bfs_fri_query(void* session, void* ps, uint32_t num_colinearity_tests, uint64_t* h_top_level_indices, void* stream) {
    return fri_query(*(FriSession*)session, *(rp::Transcript*)ps, num_colinearity_tests, h_top_level_indices, (hipStream_t)stream);
}

int bfs_fri_session_set_folding(void* session, uint32_t log2_folding) {
    FriSession* S = (FriSession*)session;
    if (log2_folding < 1 || log2_folding > 3) { set_error("bfs_fri_session_set_folding: log2_folding must be 1, 2 or 3 (got %u)", log2_folding); return BFS_ERR_BAD_ARG; }
    if (!S->rounds.empty()) { set_error("bfs_fri_session_set_folding: the session has already committed"); return BFS_ERR_BAD_ARG; }
    S->log2_folding = log2_folding;
    return BFS_OK;
}

int bfs_fri_session_set_coset_leaves(void* session, int on) {
    FriSession* S = (FriSession*)session;
    if (!S->rounds.empty()) { set_error("bfs_fri_session_set_coset_leaves: the session has already committed"); return BFS_ERR_BAD_ARG; }
    S->coset_leaves = on != 0;
    return BFS_OK;
}

int bfs_fri_session_set_grinding(void* session, uint32_t bits, uint64_t window) {
    FriSession* S = (FriSession*)session;
    if (bits > 40) { set_error("bfs_fri_session_set_grinding: bits must be in 0..40 (got %u)", bits); return BFS_ERR_BAD_ARG; }
    if (!S->rounds.empty()) { set_error("bfs_fri_session_set_grinding: the session has already committed"); return BFS_ERR_BAD_ARG; }
    S->grinding_bits = bits;
    S->grinding_window = window ? window : POW_DEFAULT_WINDOW;
    return BFS_OK;
}

static int fri_prove_run(void* ps, const uint64_t* d_codeword, uint64_t limb_stride, uint32_t log_n, uint64_t offset, uint64_t omega, uint32_t expansion_factor,
                         uint32_t log2_folding, int coset_leaves, uint32_t num_colinearity_tests, uint64_t* h_top_level_indices, void* stream) {
    FriSession S;
    S.use_workspace = true;
    BFS_TRY(bfs_fri_session_set_folding(&S, log2_folding));
    BFS_TRY(bfs_fri_session_set_coset_leaves(&S, coset_leaves));
    BFS_TRY(fri_commit(S, *(rp::Transcript*)ps, d_codeword, limb_stride, log_n, offset, omega, expansion_factor, (hipStream_t)stream));
    return fri_query(S, *(rp::Transcript*)ps, num_colinearity_tests, h_top_level_indices, (hipStream_t)stream);
}

int bfs_fri_prove(void* ps, const uint64_t* d_codeword, uint64_t limb_stride, uint32_t log_n, uint64_t offset, uint64_t omega,
                  uint32_t expansion_factor, uint32_t num_colinearity_tests, uint64_t* h_top_level_indices, void* stream) {
    return fri_prove_run(ps, d_codeword, limb_stride, log_n, offset, omega, expansion_factor, 1, 0, num_colinearity_tests, h_top_level_indices, stream);
}

int bfs_fri_prove_folded(void* ps, const uint64_t* d_codeword, uint64_t limb_stride, uint32_t log_n, uint64_t offset, uint64_t omega,
                         uint32_t expansion_factor, uint32_t log2_folding, uint32_t num_colinearity_tests, uint64_t* h_top_level_indices,
                         void* stream) {
    return fri_prove_run(ps, d_codeword, limb_stride, log_n, offset, omega, expansion_factor, log2_folding, 0, num_colinearity_tests, h_top_level_indices, stream);
}

int bfs_fri_prove_cosets(void* ps, const uint64_t* d_codeword, uint64_t limb_stride, uint32_t log_n, uint64_t offset, uint64_t omega,
                         uint32_t expansion_factor, uint32_t log2_folding, int coset_leaves, uint32_t num_colinearity_tests,
                         uint64_t* h_top_level_indices, void* stream) {
    return fri_prove_run(ps, d_codeword, limb_stride, log_n, offset, omega, expansion_factor, log2_folding, coset_leaves, num_colinearity_tests,
                         h_top_level_indices, stream);
}

// The openings of BrainfuckStark.prove (brainfuck_stark.py:315-333) written into the transcript without a Python object in between:
// for every sampled index and every distance d in (0, unit distances...): the base row at index + d, its (salt, path), the extension
// row, its (salt, path); then for every index the combination leaf and its path.  Everything the GPU holds -- row words, salts made
// on the device, tree nodes -- comes back through ONE gather; the objects are built here with the identities the reference's objects
// have (pickle memoises by identity): a row opened twice is one tuple object, a tree node or a salt one bytes object however often it
// appears, every (salt, path) tuple and path list is new, extension elements of a column whose interpolant has all its non-zero
// coefficients at multiples of 2^v share their coefficient objects with the rows i' = i mod modulus (table.ext_sharing_moduli).
//
// log2_coset = 0: the combination tree has one leaf per element, as above.  log2_coset = k in 1..3 (bfs_stark_push_openings_cosets): the
// tree is bfs_merkle_build_xfe_cosets' over cosets of a = 2^k, q = n / a leaves; for index i the coset c = i mod q is opened -- the
// tuple (C[c], C[c + q], .., C[c + (a - 1) q]), then one path of log2 q digests.  The a limb triples of every opened coset are a more
// requests of the same single gather.  One tuple object per coset: a coset that two indices share (the same index twice, or two
// indices that agree mod q) is pushed twice as the same object; the elements of a tuple are its own; a path list is new every time,
// its digests one bytes object each per tree node, like the rows' paths.  No handles go out: FRI in this form opens whole cosets itself.
static int stark_push_openings(void* ps_, const bfs_gather_request* base_row, uint32_t n_base_req, int32_t base_field_id,
                               const bfs_gather_request* ext_row, uint32_t n_ext_req, const uint64_t* ext_moduli, uint32_t n_ext_cols,
                               uint64_t n, const uint8_t* d_base_nodes, const uint8_t* base_salts, int base_salts_on_device,
                               const uint8_t* d_ext_nodes, const uint8_t* ext_salts, int ext_salts_on_device,
                               const uint64_t* d_combination, uint64_t combination_stride, const uint8_t* d_combination_nodes,
                               uint32_t log2_coset, const uint64_t* indices, uint32_t n_indices, const uint64_t* distances,
                               uint32_t n_distances, uint64_t* out_leaf_handles, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    rp::Transcript& ps = *(rp::Transcript*)ps_;
    if (n == 0 || (n & (n - 1))) { set_error("bfs_stark_push_openings: n must be a power of two"); return BFS_ERR_BAD_ARG; }
    if (log2_coset > 3 || (log2_coset && (n >> log2_coset) < 2)) { set_error("bfs_stark_push_openings_cosets: cosets of 2^%u in a codeword of %llu", log2_coset, (unsigned long long)n); return BFS_ERR_BAD_ARG; }
    if (combination_stride < n || combination_stride >> 32) { set_error("bfs_stark_push_openings: combination stride"); return BFS_ERR_BAD_ARG; }
    const u32 fan = 1u << log2_coset;                   // elements per opened leaf of the combination tree
    const u64 comb_leaves = n >> log2_coset;            // leaves of that tree
    u32 base_words = 0, ext_words = 0;
    for (u32 k = 0; k < n_base_req; ++k) base_words += base_row[k].nwords;
    for (u32 k = 0; k < n_ext_req; ++k) ext_words += ext_row[k].nwords;
    if (base_words < 3 || ext_words != 3 * n_ext_cols) { set_error("bfs_stark_push_openings: row layout"); return BFS_ERR_BAD_ARG; }
    // unique rows in order of first use, unique indices
    std::vector<u64> rows, uniq_idx;
    for (u32 a = 0; a < n_indices; ++a) {
        for (u32 b = 0; b < n_distances; ++b) {
            const u64 r = (indices[a] + distances[b]) % n;
            if (std::find(rows.begin(), rows.end(), r) == rows.end()) rows.push_back(r);
        }
        if (indices[a] >= n) { set_error("bfs_stark_push_openings: index %llu outside the domain", (unsigned long long)indices[a]); return BFS_ERR_BAD_ARG; }
        const u64 leaf = indices[a] & (comb_leaves - 1);          // the opened leaf: the index itself, or its coset
        if (std::find(uniq_idx.begin(), uniq_idx.end(), leaf) == uniq_idx.end()) uniq_idx.push_back(leaf);
    }
    // ---- one gather
    std::vector<GatherReq> reqs;
    u64 nwords = 0;
    auto want = [&](const u64* base, u32 words, u32 stride) { reqs.push_back(GatherReq{base, words, stride, nwords}); const u64 at = nwords; nwords += words; return at; };
    struct RowAt { u64 base, ext, base_salt, ext_salt; };
    std::vector<RowAt> row_at(rows.size());
    typedef FriSession::Key Key;
    FriSession::KeyMap node_at[3];                      // (tree, heap index) -> offset of the digest in the gathered words (stored as a K_INT node)
    std::vector<std::pair<int, u64>> node_list;        // order of first use
    std::vector<u64> node_off;
    const uint8_t* tree_nodes[3] = {d_base_nodes, d_ext_nodes, d_combination_nodes};
    const u64 tree_leaves[3] = {n, n, comb_leaves};
    auto want_path = [&](int tree, u64 leaf) {
        for (u64 k = tree_leaves[tree] | leaf; k > 1; k >>= 1) {
            const Key key(0, k ^ 1);
            if (node_at[tree].count(key)) continue;
            node_at[tree][key] = rp::mk_int(node_off.size());
            node_list.push_back({tree, k ^ 1});
            node_off.push_back(want((const u64*)(tree_nodes[tree] + 64 * (k ^ 1)), 8, 1));
        }
    };
    for (size_t r = 0; r < rows.size(); ++r) {
        const u64 i = rows[r];
        row_at[r].base = nwords;
        for (u32 k = 0; k < n_base_req; ++k) want(base_row[k].d_base + i, base_row[k].nwords, base_row[k].stride);
        row_at[r].ext = nwords;
        for (u32 k = 0; k < n_ext_req; ++k) want(ext_row[k].d_base + i, ext_row[k].nwords, ext_row[k].stride);
        row_at[r].base_salt = base_salts_on_device ? want((const u64*)(base_salts + 24 * i), 3, 1) : 0;
        row_at[r].ext_salt = ext_salts_on_device ? want((const u64*)(ext_salts + 24 * i), 3, 1) : 0;
        want_path(0, i);
        want_path(1, i);
    }
    std::vector<u64> leaf_at(uniq_idx.size());
    for (size_t a = 0; a < uniq_idx.size(); ++a) {
        leaf_at[a] = nwords;                            // `fan` limb triples, one behind the other
        for (u32 j = 0; j < fan; ++j) want(d_combination + uniq_idx[a] + j * comb_leaves, 3, (u32)combination_stride);
        want_path(2, uniq_idx[a]);
    }
    PinnedLease req_area, res_area;
    const u64* words = nullptr;
    BFS_TRY(gather_run(reqs, nwords, stream, req_area, res_area, &words));
    // ---- objects
    std::vector<rp::Ref> node_obj(node_list.size());
    for (size_t k = 0; k < node_list.size(); ++k) node_obj[k] = rp::mk_bytes(words + node_off[k], 64);
    auto path_obj = [&](int tree, u64 leaf) {
        std::vector<rp::Ref> items;
        for (u64 k = tree_leaves[tree] | leaf; k > 1; k >>= 1) items.push_back(node_obj[node_at[tree][Key(0, k ^ 1)]->ival]);
        return rp::mk_list(items);
    };
    const rp::Ref base_field = ps.world.base_field(base_field_id);
    std::vector<rp::Ref> base_rows(rows.size()), ext_rows(rows.size()), base_salt_obj(rows.size()), ext_salt_obj(rows.size());
    std::vector<FriSession::KeyMap> shared(n_ext_cols);          // per column: i mod modulus -> list node holding the coefficient objects
    for (size_t r = 0; r < rows.size(); ++r) {
        const u64 i = rows[r];
        const u64* bw = words + row_at[r].base;
        std::vector<rp::Ref> items;
        u64 l[3] = {bw[0], bw[1], bw[2]};
        items.push_back(ps.world.xfe_compact(l));                                    // the randomizer codeword's element
        for (u32 k = 3; k < base_words; ++k) items.push_back(ps.world.bfe_in(bw[k], base_field));
        base_rows[r] = rp::mk_tuple(items);
        const u64* ew = words + row_at[r].ext;
        items.clear();
        for (u32 c = 0; c < n_ext_cols; ++c) {
            u64 e[3] = {ew[3 * c], ew[3 * c + 1], ew[3 * c + 2]};
            if (ext_moduli[c] == 0) { items.push_back(ps.world.xfe_compact(e)); continue; }
            const Key cls(0, i % ext_moduli[c]);
            if (!shared[c].count(cls)) {
                const int k = e[2] ? 3 : (e[1] ? 2 : (e[0] ? 1 : 0));
                std::vector<rp::Ref> coeffs;
                for (int j = 0; j < k; ++j) coeffs.push_back(ps.world.bfe(e[j], true));
                shared[c][cls] = rp::mk_list(coeffs);
            }
            items.push_back(ps.world.xfe_from(shared[c][cls]->items));
        }
        ext_rows[r] = rp::mk_tuple(items);
        base_salt_obj[r] = base_salts_on_device ? rp::mk_bytes(words + row_at[r].base_salt, 24) : rp::mk_bytes(base_salts + 24 * i, 24);
        ext_salt_obj[r] = ext_salts_on_device ? rp::mk_bytes(words + row_at[r].ext_salt, 24) : rp::mk_bytes(ext_salts + 24 * i, 24);
    }
    // ---- pushes, in the reference's order
    for (u32 a = 0; a < n_indices; ++a)
        for (u32 b = 0; b < n_distances; ++b) {
            const u64 i = (indices[a] + distances[b]) % n;
            const size_t r = (size_t)(std::find(rows.begin(), rows.end(), i) - rows.begin());
            ps.objects.push_back(base_rows[r]);
            ps.objects.push_back(rp::mk_tuple({base_salt_obj[r], path_obj(0, i)}));
            ps.objects.push_back(ext_rows[r]);
            ps.objects.push_back(rp::mk_tuple({ext_salt_obj[r], path_obj(1, i)}));
        }
    std::vector<rp::Ref> leaf_obj(uniq_idx.size());
    for (size_t a = 0; a < uniq_idx.size(); ++a) {
        std::vector<rp::Ref> items;
        for (u32 j = 0; j < fan; ++j) {
            const u64* w = words + leaf_at[a] + 3 * j;
            u64 l[3] = {w[0], w[1], w[2]};
            items.push_back(ps.world.xfe_compact(l));
        }
        leaf_obj[a] = log2_coset ? rp::mk_tuple(items) : items[0];
    }
    for (u32 a = 0; a < n_indices; ++a) {
        const u64 leaf = indices[a] & (comb_leaves - 1);
        const size_t u = (size_t)(std::find(uniq_idx.begin(), uniq_idx.end(), leaf) - uniq_idx.begin());
        ps.objects.push_back(leaf_obj[u]);
        ps.objects.push_back(path_obj(2, leaf));
        if (out_leaf_handles) out_leaf_handles[a] = ps.add(leaf_obj[u]);
    }
    return BFS_OK;
}

int bfs_stark_push_openings(void* ps, const bfs_gather_request* base_row, uint32_t n_base_req, int32_t base_field_id,
                            const bfs_gather_request* ext_row, uint32_t n_ext_req, const uint64_t* ext_moduli, uint32_t n_ext_cols,
                            uint64_t n, const uint8_t* d_base_nodes, const uint8_t* base_salts, int base_salts_on_device,
                            const uint8_t* d_ext_nodes, const uint8_t* ext_salts, int ext_salts_on_device,
                            const uint64_t* d_combination, uint64_t combination_stride, const uint8_t* d_combination_nodes,
                            const uint64_t* indices, uint32_t n_indices, const uint64_t* distances, uint32_t n_distances,
                            uint64_t* out_leaf_handles, void* stream) {
    return stark_push_openings(ps, base_row, n_base_req, base_field_id, ext_row, n_ext_req, ext_moduli, n_ext_cols, n, d_base_nodes, base_salts,
                               base_salts_on_device, d_ext_nodes, ext_salts, ext_salts_on_device, d_combination, combination_stride,
                               d_combination_nodes, 0, indices, n_indices, distances, n_distances, out_leaf_handles, stream);
}

int bfs_stark_push_openings_cosets(void* ps, const bfs_gather_request* base_row, uint32_t n_base_req, int32_t base_field_id,
                                   const bfs_gather_request* ext_row, uint32_t n_ext_req, const uint64_t* ext_moduli, uint32_t n_ext_cols,
                                   uint64_t n, const uint8_t* d_base_nodes, const uint8_t* base_salts, int base_salts_on_device,
                                   const uint8_t* d_ext_nodes, const uint8_t* ext_salts, int ext_salts_on_device,
                                   const uint64_t* d_combination, uint64_t combination_stride, const uint8_t* d_combination_nodes,
                                   uint32_t log2_coset, const uint64_t* indices, uint32_t n_indices, const uint64_t* distances,
                                   uint32_t n_distances, void* stream) {
    if (log2_coset < 1) { set_error("bfs_stark_push_openings_cosets: log2_coset must be 1, 2 or 3 (got %u)", log2_coset); return BFS_ERR_BAD_ARG; }
    return stark_push_openings(ps, base_row, n_base_req, base_field_id, ext_row, n_ext_req, ext_moduli, n_ext_cols, n, d_base_nodes, base_salts,
                               base_salts_on_device, d_ext_nodes, ext_salts, ext_salts_on_device, d_combination, combination_stride,
                               d_combination_nodes, log2_coset, indices, n_indices, distances, n_distances, nullptr, stream);
}

int bfs_gather(const bfs_gather_request* requests, uint32_t count, uint64_t* h_out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (count == 0) return BFS_OK;
    static_assert(sizeof(bfs_gather_request) == sizeof(GatherReq), "layout of bfs_gather_request");
    u64 nwords = 0;
    std::vector<GatherReq> reqs(count);
    for (uint32_t i = 0; i < count; ++i) {
        reqs[i] = GatherReq{requests[i].d_base, requests[i].nwords, requests[i].stride, nwords};
        nwords += requests[i].nwords;
    }
    PinnedLease req_area, res_area;
    const u64* words = nullptr;
    BFS_TRY(gather_run(reqs, nwords, stream, req_area, res_area, &words));
    memcpy(h_out, words, nwords * sizeof(u64));
    return BFS_OK;
}

// leaves: 0 for a tree over single elements (as many leaves as the codeword is long), else the leaves of a coset tree
static int session_round0_tree(FriSession* S, const uint8_t* d_nodes, uint64_t leaves, const uint8_t h_root[64]) {
    S->round0_nodes = (const u64*)d_nodes;
    S->round0_leaves = leaves;
    memcpy(S->round0_root, h_root, 64);
    return BFS_OK;
}

int bfs_fri_session_round0_tree(void* session, const uint8_t* d_nodes, const uint8_t h_root[64]) {
    return session_round0_tree((FriSession*)session, d_nodes, 0, h_root);
}

int bfs_fri_session_round0_coset_tree(void* session, const uint8_t* d_nodes, uint64_t num_leaves, const uint8_t h_root[64]) {
    if (num_leaves == 0 || (num_leaves & (num_leaves - 1))) { set_error("bfs_fri_session_round0_coset_tree: %llu leaves", (unsigned long long)num_leaves); return BFS_ERR_BAD_ARG; }
    return session_round0_tree((FriSession*)session, d_nodes, num_leaves, h_root);
}

int bfs_fri_session_alias(void* session, void* ps, uint32_t round, uint64_t index, uint64_t element_handle) {
    rp::Ref r = ((rp::Transcript*)ps)->get(element_handle);
    if (!r) { set_error("bfs_fri_session_alias: unknown object handle"); return BFS_ERR_BAD_ARG; }
    if (((FriSession*)session)->coset_leaves) {
        set_error("bfs_fri_session_alias: a session that commits to cosets opens whole cosets; the caller cannot hold elements of one it has not opened");
        return BFS_ERR_BAD_ARG;
    }
    ((FriSession*)session)->elements[FriSession::Key(round, index)] = r;
    return BFS_OK;
}

void bfs_fri_last_timing(double out[6]) { for (int i = 0; i < 6; ++i) out[i] = g_fri_timing[i]; }

uint32_t bfs_fri_session_rounds(void* session) { return (uint32_t)((FriSession*)session)->rounds.size(); }

int bfs_fri_session_round(void* session, uint32_t r, const uint64_t** d_codeword, uint64_t* length, uint64_t* limb_stride,
                          const uint8_t** d_nodes, uint8_t h_root[64]) {
    FriSession* S = (FriSession*)session;
    if (r >= S->rounds.size()) { set_error("round %u out of range", r); return BFS_ERR_BAD_ARG; }
    const FriRound& fr = S->rounds[r];
    *d_codeword = fr.cw; *length = fr.length; *limb_stride = fr.stride; *d_nodes = (const uint8_t*)fr.nodes;     // (fr.leaves leaves: bfs_fri_session_round_leaves)
    memcpy(h_root, fr.root, 64);
    return BFS_OK;
}

uint64_t bfs_fri_session_round_leaves(void* session, uint32_t r) {
    FriSession* S = (FriSession*)session;
    return r < S->rounds.size() ? S->rounds[r].leaves : 0;
}

// what bfs_xfe_fold and bfs_xfe_fold_multi share once each has checked its own arguments: the order of omega, the constants, the launch
static int xfe_fold_run(const uint64_t* d_in, uint64_t in_stride, uint64_t* d_out, uint64_t out_stride, uint32_t log_n, uint32_t log2_folding,
                        const uint64_t alpha[3], uint64_t offset, uint64_t omega, void* stream) {
    const u64 N = 1ull << log_n;
    if (gl_pow(omega, N) != 1 || gl_pow(omega, N / 2) == 1) { set_error("error in commit: omega does not have the right order!"); return BFS_ERR_NOT_ROOT; }
    const u64 *lo = nullptr, *hi = nullptr;
    u32 lo_bits = 0;
    BFS_TRY(ntt_power_tables(gl_inv(omega), log_n, &lo, &hi, &lo_bits));
    Xfe a{{alpha[0] % GL_P, alpha[1] % GL_P, alpha[2] % GL_P}};
    FriFoldArgs f{};
    f.in = d_in; f.in_stride = in_stride;
    f.winv_lo = lo; f.winv_hi = hi; f.lo_bits = lo_bits; f.round_shift = 0;
    fri_fold_constants(f, log2_folding, N, a, offset % GL_P, omega);
    return fri_fold_launch(f, d_out, out_stride, (hipStream_t)stream);
}

int bfs_xfe_fold(const uint64_t* d_in, uint64_t in_stride, uint64_t* d_out, uint64_t out_stride, uint32_t log_n, const uint64_t alpha[3],
                 uint64_t offset, uint64_t omega, void* stream) {
    if (log_n == 0) { set_error("cannot fold a codeword of length 1"); return BFS_ERR_BAD_ARG; }
    return xfe_fold_run(d_in, in_stride, d_out, out_stride, log_n, 1, alpha, offset, omega, stream);
}

int bfs_xfe_fold_multi(const uint64_t* d_in, uint64_t in_stride, uint64_t* d_out, uint64_t out_stride, uint32_t log_n, uint32_t log2_folding,
                       const uint64_t alpha[3], uint64_t offset, uint64_t omega, void* stream) {
    const u64 N = 1ull << log_n;
    if (log2_folding < 1 || log2_folding > 3) { set_error("bfs_xfe_fold_multi: log2_folding must be 1, 2 or 3 (got %u)", log2_folding); return BFS_ERR_BAD_ARG; }
    if (log_n < log2_folding || log_n > 32) { set_error("cannot fold a codeword of length 2^%u by %u", log_n, 1u << log2_folding); return BFS_ERR_BAD_ARG; }
    if (in_stride < N || out_stride < (N >> log2_folding)) { set_error("bfs_xfe_fold_multi: a limb stride is shorter than its codeword"); return BFS_ERR_BAD_ARG; }
    return xfe_fold_run(d_in, in_stride, d_out, out_stride, log_n, log2_folding, alpha, offset, omega, stream);
}

}  // extern "C"
