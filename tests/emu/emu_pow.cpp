// Host emulation of the proof-of-work search kernel (csrc/pow.hip over csrc/pow_core.hpp): every lane of a simulated launch runs the
// kernel's per-lane scan, and the launch's result is the minimum over the lanes, as the kernel's atomicMin leaves it.
// TEST INFRASTRUCTURE, see emu_ntt.cpp.
#include <cstring>

#include "../../stark_brainfuck_amd/csrc/pow_core.hpp"

using namespace bfs;

// -> the smallest hit in [first, first + count) as `lanes` lanes find it (*found = 0: none); -2: a lane answered a nonce that is not one
// of its own
extern "C" int emu_pow_search(const unsigned char seed[32], unsigned bits, u64 first, u64 count, u64 lanes, u64* nonce, int* found) {
    if (bits < 1 || bits > 64 || lanes == 0 || count == 0 || first + (count - 1) < first) return -1;
    u64 words[4];
    memcpy(words, seed, 32);
    u64 best = POW_NO_HIT;
    for (u64 lane = 0; lane < lanes; ++lane) {
        const u64 got = pow_scan_lane(words, bits, first, count, lane, lanes);
        if (got != POW_NO_HIT) {
            if (got < first || got - first >= count || (got - first) % lanes != lane) return -2;     // not one of this lane's nonces
            if (got < best) best = got;
        }
    }
    *found = best != POW_NO_HIT;
    *nonce = best;
    return 0;
}

extern "C" int emu_pow_hit(const unsigned char seed[32], u64 nonce, unsigned bits) {
    u64 words[4];
    memcpy(words, seed, 32);
    return pow_hit(words, nonce, bits) ? 1 : 0;
}
