"""The cases and the integer models of the two blinding entries of include/bfstark_blind.h, shared by tests/test_gpu_blind_kernels.py (the
kernels on the MI355X), tests/test_blind_emulation.py (the same per-word bodies compiled for the host) and tests/blind_stream_child.py.
The models are Python integers throughout; operands come from the palette of tests/field_states.py, the blinding words also from values
>= p up to 2^64 - 1, laid out with coprime periods so that every pairing of a coefficient and a blinding word occurs."""
import itertools

import numpy as np

from field_states import P, PALETTE

M64 = (1 << 64) - 1
BLIND_PALETTE = PALETTE + (P, P + 1, 0xFFFFFFFF80000000, M64)          # 19 words: 15 residues, four values >= p
assert len(BLIND_PALETTE) == 19 and sum(v >= P for v in BLIND_PALETTE) == 4

POLY_HEIGHTS, POLY_BLINDS, POLY_BATCHES = (1, 2, 64, 4096), (1, 8, 14, 70), (1, 27, 300)
POLY_CASES = [(h, k, batch, slack) for h, k, batch in itertools.product(POLY_HEIGHTS, POLY_BLINDS, POLY_BATCHES) for slack in (0, 5)]
SPLIT_CASES = [(8, 3, 2, 3), (256, 30, 2, 9), (512, 47, 17, 11), (64, 64, 0, 1), (16, 1, 1, 16)]          # (S, L0, m, s)


def poly_operands(h, k, batch):
    """(coefficients, blinding words): batch rows of h + k and of k words"""
    coefficients = [[PALETTE[(7 * b + i) % 15] for i in range(h + k)] for b in range(batch)]
    blinding = [[BLIND_PALETTE[(3 * b + 5 * i + i // 19) % 19] for i in range(k)] for b in range(batch)]
    return coefficients, blinding


def poly_blind_model(old, r, h, k, events=None):
    """one row: new[i] = old[i] - (i < k ? r[i] : 0) + (i >= h ? r[i - h] : 0) mod p.  events: a dict that counts the words whose
    subtraction borrowed / whose addition carried past p, by region -- "low" (i < k only), "high" (i >= h only), "both" (h <= i < k)"""
    out = []
    for i in range(h + k):
        a = r[i] % P if i < k else 0
        b = r[i - h] % P if i >= h else 0
        out.append((old[i] - a + b) % P)
        if events is not None:
            region = "both" if h <= i < k else "low" if i < k else "high" if i >= h else "none"
            borrow = old[i] < a
            carry = (old[i] - a) % P + b >= P
            for name, hit in (("borrow", borrow), ("carry", carry), ("borrow and carry", borrow and carry)):
                if hit:
                    events[region, name] = events.get((region, name), 0) + 1
    return out


def split_operands(S, L0, m, s, seed=0):
    """(H, b): H three planes of S words, b[j][l] m words for j < s - 1"""
    H = [[BLIND_PALETTE[(seed + 11 * l + 4 * i + i // 19) % 19] for i in range(S)] for l in range(3)]
    b = [[[BLIND_PALETTE[(seed + 2 * j + 7 * l + 3 * c) % 19] for c in range(m)] for l in range(3)] for j in range(max(s - 1, 0))]
    return H, b


def split_blind_model(H, S, L0, s, b, m):
    """out[j][l][c] for c < L0 + m, by the header's formula"""
    out = []
    for j in range(s):
        out.append([])
        for l in range(3):
            row = []
            for c in range(L0 + m):
                v = H[l][j * L0 + c] if c < L0 and j * L0 + c < S else 0
                if c >= L0 and j < s - 1:
                    v += b[j][l][c - L0]
                if c < m and j >= 1:
                    v -= b[j - 1][l][c]
                row.append(v % P)
            out[-1].append(row)
    return out


def recombined(out, L0, s):
    """sum_j X^(j L0) out_j per limb plane, as coefficient lists mod p"""
    width = len(out[0][0])
    planes = []
    for l in range(3):
        total = [0] * ((s - 1) * L0 + width)
        for j in range(s):
            for c, v in enumerate(out[j][l]):
                total[j * L0 + c] = (total[j * L0 + c] + v) % P
        planes.append(total)
    return planes


def strided(rows, stride, fill):
    """rows of words `stride` apart in one uint64 array, `fill` in the gaps"""
    out = np.full(len(rows) * stride, fill, dtype=np.uint64)
    for k, row in enumerate(rows):
        out[k * stride:k * stride + len(row)] = np.array(row, dtype=np.uint64)
    return out
