// blind_core.hpp -- the per-word bodies of the two blinding kernels of the zero-knowledge mode of prove_deep (include/bfstark_blind.h;
// DESIGN.md, "Zero-knowledge openings"), host/device code: the kernels (csrc/blind.hip) and the CPU emulation (tests/emu/emu_blind.cpp)
// call these very functions, one call per output word.  Each word is computed from the OLD contents of its own position and from read-only
// blinding words, so the order of the threads does not matter and a blinding polynomial longer than the trace (k > h) cannot race.
#pragma once
#include "gl.hpp"

namespace bfs {

// coefficient i < h + k of f + (X^h - 1) r, from coefficient i of f (zero for i >= the interpolant's length) and the k words of r:
// old - (i < k ? r[i] : 0) + (i >= h ? r[i - h] : 0).  Blinding words are any 64-bit values and are reduced; `old` is canonical.
BFS_HD u64 poly_blind_word(u64 old, const u64* r, u64 i, u64 h, u64 k) {
    u64 v = old;
    if (i < k) v = gl_sub(v, gl_canon(r[i]));
    if (i >= h) v = gl_add(v, gl_canon(r[i - h]));
    return v;
}

// word c < L0 + m of limb plane l of blinded segment j < s of H (S coefficients per plane, planes h_stride apart):
//   (c < L0 and j L0 + c < S ? H[l][j L0 + c] : 0) + (c >= L0 and j < s - 1 ? b[j][l][c - L0] : 0) - (c < m and j >= 1 ? b[j - 1][l][c] : 0)
// with b[j][l] = d_b + (3 j + l) * b_stride, m words each (m <= L0: a word takes at most one of the first two terms)
BFS_HD u64 split_blind_word(const u64* hp, u64 h_stride, u64 S, u64 L0, u32 s, const u64* b, u64 b_stride, u64 m, u32 j, u32 l, u64 c) {
    u64 v = 0;
    if (c < L0) {
        const u64 at = (u64)j * L0 + c;
        if (at < S) v = gl_canon(hp[l * h_stride + at]);
    } else if (j + 1 < s) {
        v = gl_canon(b[(3 * (u64)j + l) * b_stride + (c - L0)]);
    }
    if (c < m && j >= 1) v = gl_sub(v, gl_canon(b[(3 * (u64)(j - 1) + l) * b_stride + c]));
    return v;
}

}  // namespace bfs
