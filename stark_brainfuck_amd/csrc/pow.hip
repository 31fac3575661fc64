// pow.hip -- proof-of-work grinding for Fri(..., grinding_bits=b): the search for the smallest nonce n with
// blake2b(seed || n) starting with b zero bits (pow_core.hpp), on gfx950.  Register-only integer work: no LDS, no loads, one
// atomicMin per lane that found something.  Every launch is a bounded amount of work -- at most POW_PER_THREAD hashes per thread,
// no waiting on other threads, no flag that ends it early; the host looks at the result between launches and stops at the first
// launch with a hit, which holds the window's smallest hit because the launches ascend.
#include "../../include/bfstark.h"
#include "pow_core.hpp"
#include "runtime.hpp"

namespace bfs {

constexpr u32 POW_BLOCK = 256;
constexpr u32 POW_PER_THREAD = 16;                 // nonces a thread scans at most, POW_BLOCK * gridDim.x apart
constexpr u64 POW_LAUNCH_MIN = (u64)POW_BLOCK * POW_PER_THREAD;   // one workgroup's share
constexpr u64 POW_LAUNCH_MAX = 1ULL << 24;         // nonces per launch: 4096 workgroups, a millisecond or two of hashing

struct PowSeed {
    u64 w[4];
};

// lane = global thread index, lanes = threads of the launch; count <= lanes * POW_PER_THREAD.  *result starts at POW_NO_HIT (the caller's
// job) and ends as the smallest hit in [first, first + count) -- a hit at 2^64 - 1 leaves it as it is, see pow_search.
__global__ void __launch_bounds__(POW_BLOCK) pow_search_kernel(PowSeed seed, u32 bits, u64 first, u64 count, u64* result) {
    const u64 lanes = (u64)gridDim.x * POW_BLOCK;
    const u64 lane = (u64)blockIdx.x * POW_BLOCK + threadIdx.x;
    const u64 nonce = pow_scan_lane(seed.w, bits, first, count, lane, lanes);
    if (nonce != POW_NO_HIT) atomicMin((unsigned long long*)result, (unsigned long long)nonce);
}

static void seed_words(const uint8_t seed[32], u64 w[4]) { memcpy(w, seed, 32); }      // little-endian host

// the smallest hit in [first, first + count), count >= 1 and first + count <= 2^64.  A launch takes 2^(bits + 2) nonces (four hits
// expected, so a few lanes meet at the result word instead of half the launch when bits is small), at least POW_LAUNCH_MIN and at most
// POW_LAUNCH_MAX.  Synchronises the stream after every launch.
int pow_search(const u64 seed[4], u32 bits, u64 first, u64 count, u64* nonce, bool* found, hipStream_t stream) {
    *found = false;
    u64 step = bits + 2 >= 24 ? POW_LAUNCH_MAX : 1ULL << (bits + 2);
    if (step < POW_LAUNCH_MIN) step = POW_LAUNCH_MIN;
    PowSeed s;
    memcpy(s.w, seed, sizeof s.w);
    void* d_result = nullptr;
    PinnedLease back;
    BFS_TRY(back.get(sizeof(u64)));
    BFS_TRY(device_alloc(sizeof(u64), stream, &d_result));
    int rc = BFS_OK;
    hipError_t e = hipMemsetAsync(d_result, 0xFF, sizeof(u64), stream);
    for (u64 done = 0; e == hipSuccess && done < count; done += step) {
        const u64 n = count - done < step ? count - done : step;
        const u32 grid = (u32)((n + POW_LAUNCH_MIN - 1) / POW_LAUNCH_MIN);
        hipLaunchKernelGGL(pow_search_kernel, dim3(grid), dim3(POW_BLOCK), 0, stream, s, bits, first + done, n, (u64*)d_result);
        if ((e = hipGetLastError()) != hipSuccess) break;
        if ((e = hipMemcpyAsync(back.host, d_result, sizeof(u64), hipMemcpyDeviceToHost, stream)) != hipSuccess) break;
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) break;
        const u64 got = *(const volatile u64*)back.host;
        if (got != POW_NO_HIT) { *nonce = got; *found = true; break; }
    }
    if (e != hipSuccess) { set_error("pow_search: %s", hipGetErrorString(e)); rc = BFS_ERR_HIP; }
    (void)device_release(d_result, stream);
    if (rc == BFS_OK && !*found && first + (count - 1) == POW_NO_HIT && pow_hit(seed, POW_NO_HIT, bits)) {
        *nonce = POW_NO_HIT;       // the one nonce that looks like "nothing found" to the kernel
        *found = true;
    }
    return rc;
}

}  // namespace bfs

using namespace bfs;

extern "C" {

int bfs_pow_check(const uint8_t seed[32], uint32_t bits, uint64_t nonce, int* ok) {
    if (!seed || !ok) { set_error("bfs_pow_check: null argument"); return BFS_ERR_BAD_ARG; }
    if (bits < 1 || bits > POW_MAX_BITS) { set_error("bfs_pow_check: bits must be in 1..%u (got %u)", POW_MAX_BITS, bits); return BFS_ERR_BAD_ARG; }
    u64 w[4];
    seed_words(seed, w);
    *ok = pow_hit(w, nonce, bits) ? 1 : 0;
    return BFS_OK;
}

int bfs_pow_search(const uint8_t seed[32], uint32_t bits, uint64_t first_nonce, uint64_t count, uint64_t* nonce, int* found, void* stream) {
    if (!seed || !nonce || !found) { set_error("bfs_pow_search: null argument"); return BFS_ERR_BAD_ARG; }
    if (bits < 1 || bits > POW_MAX_BITS) { set_error("bfs_pow_search: bits must be in 1..%u (got %u)", POW_MAX_BITS, bits); return BFS_ERR_BAD_ARG; }
    if (count == 0) { set_error("bfs_pow_search: an empty window"); return BFS_ERR_BAD_ARG; }
    if (first_nonce + (count - 1) < first_nonce) { set_error("bfs_pow_search: the window wraps 2^64"); return BFS_ERR_BAD_ARG; }
    u64 w[4];
    seed_words(seed, w);
    bool hit = false;
    u64 n = 0;
    BFS_TRY(pow_search(w, bits, first_nonce, count, &n, &hit, (hipStream_t)stream));
    *found = hit ? 1 : 0;
    if (hit) *nonce = n;
    return BFS_OK;
}

}  // extern "C"
