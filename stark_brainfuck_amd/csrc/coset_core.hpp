// coset_core.hpp -- the per-lane half of the coset-leaf kernels (coset.hip): the Merkle leaf of a FRI round that commits one leaf per
// folding coset,
//     blake2b(pickle.dumps((C[c], C[c + q], .., C[c + (a - 1) q])))          /root/reference/code/merkle.py:29-32 on a list of tuples
// streamed into BLAKE2b element by element.  Host/device, so that tests/emu/emu_coset.cpp can run it against hashlib.
//
// Shape of the pickle when every element stores three coefficients (top limb non-zero -- every element of a folded codeword, but for
// a chance of 2^-64): element 0 is the stand-alone pickle of an element (pickle_templates.hpp) behind the tuple's MARK (TUPLE2 needs
// none), and it memoises every class, name and field object; each later element is 79 constant bytes of back-references around its three
// integers; then TUPLE2 / TUPLE, MEMOIZE, STOP.  Any other tuple (an element with a zero top limb) has another skeleton: the kernel
// reports it and the host hashes the tree with the zipped-row interpreter (rows.hip), which knows every pattern.
//
// A lane owns COSET_LANE_BYTES of LDS and writes with unaligned 8-byte stores at its own byte position (rows_core.hpp: row_store8).
// The stream is cut into STAGES of at most COSET_STAGE_MAX bytes, each straight-line code; between two stages the wave passes the one
// compression site.  The buffer is a block plus one stage, so a lane cannot wait: once it holds more than a block (pos > COSET_FORCE
// = 128) the next stage would not fit, and it compresses.  Only a lane at exactly 128 bytes waits for the lanes behind it.  Lanes
// whose integers differ in length therefore cross a block boundary at different stages, and the site then runs under a partial mask:
// up to twice per stage boundary instead of once.  (Elements of a folded codeword have 8- or 9-byte limbs, so the lanes drift by at
// most 3 bytes per element and most boundaries are crossed by the whole wave at once; a buffer of two blocks would let every lane
// wait, at 24.5 KiB of LDS per wave: six workgroups per CU instead of nine.)
#pragma once
#include "blake2b.hpp"
#include "leaf_encode.hpp"
#include "rows_core.hpp"

namespace bfs {

constexpr u32 COSET_STAGE_MAX = 120;                       // bytes one stage appends at most (an element: 79 + 3 * 11, the last one + 3)
constexpr u32 COSET_LANE_BYTES = 264;                      // 128 + COSET_STAGE_MAX + 16 of slack for the zero padding of the last store; 33 words
constexpr u32 COSET_FORCE = COSET_LANE_BYTES - COSET_STAGE_MAX - 16;      // a lane further than this cannot take another stage: it compresses first
static_assert(COSET_FORCE >= 128 && COSET_LANE_BYTES % 8 == 0, "a lane that must compress holds a complete block");

// constant bytes of an element behind the first (memo indices of a first element with three coefficients)
namespace coset_tpl {
constexpr int E_PRE_LEN = 32;      // h 2 ) NEWOBJ } ( h 5 h 8 ) NEWOBJ } h 11 ] ( h 15 ) NEWOBJ } ( h 18
BFS_TPL_CONST u64 E_PRE[4] = {0x28947d9481290268ULL, 0x7d94812908680568ULL, 0x0f6828945d0b6894ULL, 0x126828947d948129ULL};
constexpr int E_POST_LEN = 15;     // h 19 h 22 u b e s b h 19 h 31 u b
BFS_TPL_CONST u64 E_POST[2] = {0x7365627516681368ULL, 0x0062751f68136862ULL};
// (between two integers of an element: tpl::XFE_MID_B, the same 16 bytes as inside a stand-alone element)
}  // namespace coset_tpl

// length of the tuple's pickle without its 3 * A integers
template <int A>
struct CosetShape {
    static constexpr u32 MARK = A > 2 ? 1u : 0u;
    static constexpr u32 ELEMENT0 = tpl::XFE_PRE_A_LEN + 1 + tpl::XFE_PRE_B_LEN + tpl::XFE_MID_A_LEN + tpl::XFE_MID_B_LEN + tpl::XFE_POST3_LEN - 1;
    static constexpr u32 ELEMENT = coset_tpl::E_PRE_LEN + 2 * tpl::XFE_MID_B_LEN + coset_tpl::E_POST_LEN;
    static constexpr u32 CONST_BYTES = 11 + MARK + ELEMENT0 + (A - 1) * ELEMENT + 3;
    static constexpr u32 STAGES = 3 + (A - 1);              // element 0 takes three
    static constexpr u32 MIN_INT_BYTES = 2 * 3 * A, MAX_INT_BYTES = 11 * 3 * A;
    static constexpr u32 BLOCK0_STATES = MAX_INT_BYTES - MIN_INT_BYTES + 1;
};

// block 0 of the pickle (constants and the frame length) for a tuple whose integers take int_bytes bytes together
template <int A>
inline void coset_block0(u32 int_bytes, unsigned char block[128]) {
    const u64 frame = (u64)CosetShape<A>::CONST_BYTES + int_bytes - 11;
    const u64 hdr = 0x80ull | (0x04ull << 8) | (0x95ull << 16) | (frame << 24);
    memcpy(block, &hdr, 8);
    memset(block + 8, 0, 3);
    u32 at = 11;
    if (A > 2) block[at++] = 0x28;
    memcpy(block + at, tpl::XFE_PRE_A, tpl::XFE_PRE_A_LEN);
    at += tpl::XFE_PRE_A_LEN;
    block[at++] = 0x28;
    memcpy(block + at, tpl::XFE_PRE_B, 128 - at);           // 3 bytes (a = 2) or 2
}

struct CosetLane {
    u64 h[8];
    u32 pos;            // bytes in the buffer
    u32 consumed;       // bytes already compressed
    u32 total;          // length of the pickle
};

BFS_HD void coset_put(CosetLane& s, unsigned char* buf, u64 data, u32 nb) {       // bytes of data above nb are zero
    row_store8(buf + s.pos, data);
    s.pos += nb;
}
template <int LEN>
BFS_HD void coset_put_const(CosetLane& s, unsigned char* buf, const u64* words) {
    BFS_UNROLL
    for (int i = 0; i < (LEN + 7) / 8; ++i) row_store8(buf + s.pos + 8 * i, words[i]);
    s.pos += LEN;
}
BFS_HD void coset_put_int(CosetLane& s, unsigned char* buf, u64 v) {
    u64 lo, hi;
    u32 len;
    row_int_opcode(v, lo, hi, len);
    row_store8(buf + s.pos, lo);
    row_store8(buf + s.pos + 8, hi);
    s.pos += len;
}

// stage `stage` of the pickle of a tuple of A elements; (c0, c1, c2) = the element the stage belongs to: element 0 for stages 0..2,
// element stage - 2 from then on
template <int A>
BFS_HD void coset_stage(CosetLane& s, unsigned char* buf, u32 stage, u64 c0, u64 c1, u64 c2) {
    if (stage == 0) {
        if (A > 2) coset_put(s, buf, (tpl::XFE_PRE_B[0] >> 16) & 0xFF, 1);       // (block 0 ends one byte earlier in the template)
        coset_put_const<tpl::XFE_PRE_B3_LEN>(s, buf, tpl::XFE_PRE_B3);
        coset_put_int(s, buf, c0);
        coset_put_const<tpl::XFE_MID_A_LEN>(s, buf, tpl::XFE_MID_A);
    } else if (stage == 1) {
        coset_put_int(s, buf, c1);
        coset_put_const<tpl::XFE_MID_B_LEN>(s, buf, tpl::XFE_MID_B);
        coset_put_int(s, buf, c2);
        coset_put_const<72>(s, buf, tpl::XFE_POST3);
    } else if (stage == 2) {
        coset_put_const<56>(s, buf, tpl::XFE_POST3 + 9);
        coset_put(s, buf, tpl::XFE_POST3[16] & 0xFFFFFFull, 3);                  // POST3 without its STOP
    } else {
        coset_put_const<coset_tpl::E_PRE_LEN>(s, buf, coset_tpl::E_PRE);
        coset_put_int(s, buf, c0);
        coset_put_const<tpl::XFE_MID_B_LEN>(s, buf, tpl::XFE_MID_B);
        coset_put_int(s, buf, c1);
        coset_put_const<tpl::XFE_MID_B_LEN>(s, buf, tpl::XFE_MID_B);
        coset_put_int(s, buf, c2);
        coset_put_const<coset_tpl::E_POST_LEN>(s, buf, coset_tpl::E_POST);
        if (stage + 1 == CosetShape<A>::STAGES) {
            coset_put(s, buf, (A == 2 ? 0x86ull : 0x74ull) | (0x94ull << 8) | (0x2eull << 16), 3);      // TUPLE2 / TUPLE, MEMOIZE, STOP
            row_store8(buf + s.pos, 0);                                                                    // zeros behind the last byte
        }
    }
}

// while the stages are still coming: a complete block that is not the last one?
BFS_HD bool coset_lane_ready(const CosetLane& s) { return s.pos >= 128 && s.consumed + 128 < s.total; }

// compress the block at the front of the buffer and move what lies behind it to the front
BFS_HD void coset_compress(CosetLane& s, unsigned char* buf, bool at_end) {
    const u64* w = (const u64*)buf;
    const bool last = at_end && s.consumed + 128 >= s.total;
    const u32 valid = last ? s.total - s.consumed : 128;
    u64 m[16];
    BFS_UNROLL
    for (int j = 0; j < 16; ++j) m[j] = (u32)(8 * j) < valid ? w[j] : 0;
    blake2b_compress(s.h, m, last ? (u64)s.total : (u64)s.consumed + 128, last);
    s.consumed += 128;
    u64* ww = (u64*)buf;
    BFS_UNROLL
    for (u32 j = 0; j < COSET_LANE_BYTES / 8 - 16; ++j)
        if (128 + 8 * j < s.pos + 8) ww[j] = ww[16 + j];          // (+ 8: the zero padding behind the last byte moves along)
    s.pos = s.pos > 128 ? s.pos - 128 : 0;
}

}  // namespace bfs
