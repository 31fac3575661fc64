// Host emulation of the coset-leaf kernel (csrc/coset.hip over csrc/coset_core.hpp): 64 simulated lanes walk the stages of the tuple
// pickle with the kernel's compression rule.  TEST INFRASTRUCTURE, see emu_ntt.cpp.
#include <cstring>
#include <vector>

#include "../../stark_brainfuck_amd/csrc/coset_core.hpp"

using namespace bfs;

template <int A>
static void wave(const u64* cw, u64 stride, u64 q, u64 first, u64* digests, unsigned char* skipped) {
    typedef CosetShape<A> Shape;
    constexpr u32 LANES = 64;
    std::vector<unsigned char> blk(COSET_LANE_BYTES * LANES + 16, 0xA5);        // (+ 16: nothing may be written there)
    CosetLane s[LANES];
    bool ok[LANES];
    for (u32 l = 0; l < LANES; ++l) {
        const u64 c = first + l;
        ok[l] = c < q;
        u32 int_bytes = 0;
        for (u32 m = 0; ok[l] && m < (u32)A; ++m) {
            const u64 at = c + m * q;
            int_bytes += pickle_int_len(cw[at]) + pickle_int_len(cw[stride + at]) + pickle_int_len(cw[2 * stride + at]);
            if (cw[2 * stride + at] == 0) { ok[l] = false; skipped[c] = 1; }
        }
        s[l].pos = 0; s[l].consumed = 128; s[l].total = Shape::CONST_BYTES + int_bytes;
        if (ok[l]) {
            unsigned char block[128];
            coset_block0<A>(int_bytes, block);
            u64 m[16];
            memcpy(m, block, 128);
            blake2b_init(s[l].h);
            blake2b_compress(s[l].h, m, 128, false);
        }
    }
    u32 stage = 0;
    bool done = false;
    while (true) {
        bool behind = false, any = false, want[LANES];
        for (u32 l = 0; l < LANES; ++l) behind |= ok[l] && s[l].pos < 128;
        for (u32 l = 0; l < LANES; ++l) {
            if (!done) want[l] = ok[l] && coset_lane_ready(s[l]) && (s[l].pos > COSET_FORCE || !behind);
            else want[l] = ok[l] && s[l].consumed < s[l].total;
            any |= want[l];
        }
        if (any) {
            for (u32 l = 0; l < LANES; ++l)
                if (want[l]) coset_compress(s[l], blk.data() + COSET_LANE_BYTES * l, done);
            continue;
        }
        if (done) break;
        for (u32 l = 0; l < LANES; ++l) {
            if (!ok[l]) continue;
            const u64 at = first + l + (stage < 3 ? 0 : (u64)(stage - 2) * q);
            coset_stage<A>(s[l], blk.data() + COSET_LANE_BYTES * l, stage, cw[at], cw[stride + at], cw[2 * stride + at]);
            if (s[l].pos + 16 > COSET_LANE_BYTES) skipped[first + l] = 2;      // a store beyond the lane's buffer
        }
        ++stage;
        done = stage == Shape::STAGES;
    }
    for (u32 l = 0; l < LANES; ++l)
        if (ok[l]) memcpy(digests + 8 * (first + l), s[l].h, 64);
    for (u32 i = 0; i < 16; ++i)
        if (blk[COSET_LANE_BYTES * LANES + i] != 0xA5) skipped[first] = 2;
}

// leaf digests of the coset tree of a limb-major codeword of q << log2_coset elements; skipped[c] = 1: the kernel leaves leaf c to the
// zipped-row interpreter (an element with a zero top limb), 2: a lane wrote outside its buffer
extern "C" int emu_coset_leaves(const u64* cw, u64 stride, u64 q, unsigned log2_coset, u64* digests, unsigned char* skipped) {
    memset(skipped, 0, q);
    for (u64 first = 0; first < q; first += 64) {
        if (log2_coset == 1) wave<2>(cw, stride, q, first, digests, skipped);
        else if (log2_coset == 2) wave<4>(cw, stride, q, first, digests, skipped);
        else if (log2_coset == 3) wave<8>(cw, stride, q, first, digests, skipped);
        else return -1;
    }
    return 0;
}
