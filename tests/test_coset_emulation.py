"""The coset-leaf kernel's per-lane code (csrc/coset_core.hpp) on the host: 64 simulated lanes walk the stages of the tuple pickle with
the kernel's compression rule (tests/emu/emu_coset.cpp); every digest against hashlib over oracle.dumps of the tuple.  No GPU."""
import ctypes
import hashlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

import fri_coset_model as model

u64, vp = ctypes.c_uint64, ctypes.c_void_p


@pytest.fixture(scope="module")
def emu():
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    from build_emu import build_emulation
    lib = ctypes.CDLL(build_emulation())
    lib.emu_coset_leaves.argtypes = [vp, u64, u64, ctypes.c_uint, vp, vp]
    return lib


def _leaves(emu, cw, q, k):
    cw = np.ascontiguousarray(cw)
    digests, skipped = np.zeros(8 * q, dtype=np.uint64), np.zeros(q, dtype=np.uint8)
    assert emu.emu_coset_leaves(cw.ctypes.data, cw.shape[1], q, k, digests.ctypes.data, skipped.ctypes.data) == 0
    return [digests[8 * c:8 * c + 8].tobytes() for c in range(q)], skipped


@pytest.mark.parametrize("a", [2, 4, 8])
@pytest.mark.parametrize("planted", [None, "full", "short"])
def test_leaf_digests(emu, oracle, a, planted):
    k = a.bit_length() - 1
    for q, pad in ((1, 0), (2, 5), (64, 0), (70, 3), (300, 0)):          # (the emulation takes any q; the kernel's callers pass powers of two)
        n = a * q
        cw = model.tree_codeword(oracle, 0xC05E + q, n, a, stride=n + pad, planted=planted)
        got, skipped = _leaves(emu, cw, q, k)
        assert not (skipped == 2).any(), "a lane wrote outside its buffer"
        left = 0
        for c in range(q):
            limbs = [[int(cw[y, c + j * q]) for y in range(3)] for j in range(a)]
            short = any(l[2] == 0 for l in limbs)
            assert skipped[c] == (1 if short else 0), (q, c)
            if short:
                left += 1
                continue
            want = hashlib.blake2b(oracle.dumps(tuple(oracle.make_xfe(l) for l in limbs))).digest()
            assert got[c] == want, (q, c)
        assert (left > 0) == (planted == "short")


def test_the_planted_codewords_hold_what_they_promise(oracle):
    for a in (2, 4, 8):
        q = 512
        full = model.tree_codeword(oracle, 1, a * q, a, planted="full")
        short = model.tree_codeword(oracle, 1, a * q, a, planted="short")
        assert (full[2, :a * q] != 0).all()
        stored = {3 - [int(short[2, i]) != 0, int(short[1, i]) != 0, int(short[0, i]) != 0, True].index(True) for i in range(a * q)}
        assert stored == {0, 1, 2, 3}
        for cw in (full, short):
            flat = {int(v) for v in cw[:, :a * q].reshape(-1)}
            assert {1, 255} <= flat and any(v >= 1 << 63 for v in flat) and any(256 <= v < 1 << 31 for v in flat)
