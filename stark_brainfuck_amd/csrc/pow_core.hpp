// pow_core.hpp -- the proof-of-work predicate of Fri(..., grinding_bits=b) and the per-lane nonce scan, host/device code: the search
// kernel (csrc/pow.hip), the host check (bfs_pow_check) and the CPU emulation (tests/emu/emu_pow.cpp) call these very functions.
//
//     hit(seed, n, b) := int.from_bytes(blake2b(seed + n.to_bytes(8, "little")).digest()[:8], "little") >> (64 - b) == 0
//
// seed: the 32 bytes of Fiat-Shamir randomness drawn after the last codeword, as four little-endian words.  The 40-byte message is one
// final compression block with t = 40: message words 0..3 the seed, word 4 the nonce, words 5..15 zero.  The eleven zero words are
// literals, so their additions fold away, and the predicate reads h[0] alone: after inlining, the compiler drops the two G's of the
// last diagonal half-round that feed neither v0 nor v8, and every h[i], i > 0.
#pragma once
#include "blake2b.hpp"

namespace bfs {

constexpr u32 POW_MAX_BITS = 40;
constexpr u64 POW_NO_HIT = ~0ULL;      // what a scan without a hit answers.  It is also the largest nonce: a caller whose window ends at
                                       // 2^64 tells "no hit" from "2^64 - 1 hits" by asking pow_hit about that one nonce (pow.hip)

// h[0] of blake2b(seed || nonce): the first eight digest bytes, little-endian
BFS_HD u64 pow_word(const u64 seed[4], u64 nonce) {
#if defined(__HIP_DEVICE_COMPILE__)
    // the scan hands over first + at: seen as a sum, the nonce lets the optimiser re-associate it with the additions of every G it
    // enters, rotations included (their halves are joined by an `or` that counts as an addition), and the kernel came out at 3 645
    // VALU instructions and 255 VGPRs.  Behind this empty statement the nonce is one value: 1 750 instructions, 64 VGPRs.
    asm("" : "+v"(nonce));
#endif
    u64 h[8];
    blake2b_init(h);
    const u64 m[16] = {seed[0], seed[1], seed[2], seed[3], nonce, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    blake2b_compress(h, m, 40, true);
    return h[0];
}

// bits in 1..64
BFS_HD bool pow_hit(const u64 seed[4], u64 nonce, u32 bits) { return (pow_word(seed, nonce) >> (64 - bits)) == 0; }

// lane `lane` of `lanes` scans the nonces first + lane + i * lanes below first + count (first + count <= 2^64: `at` counts within the
// window, so nothing wraps) in ascending order; the smallest hit, or POW_NO_HIT
BFS_HD u64 pow_scan_lane(const u64 seed[4], u32 bits, u64 first, u64 count, u64 lane, u64 lanes) {
    for (u64 at = lane; at < count;) {
        if (pow_hit(seed, first + at, bits)) return first + at;
        if (count - at <= lanes) break;
        at += lanes;
    }
    return POW_NO_HIT;
}

}  // namespace bfs
