"""The per-word bodies of the two blinding kernels (csrc/blind_core.hpp) on the host: tests/emu/emu_blind.cpp walks each launch's grid with
the kernels' guards; every word against the Python-integer models of tests/blind_cases.py, over the case lists the GPU test uses.  Also
what the case lists are for: borrows and carries in every region of a blinded row, and the segment identity on integers.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

import blind_cases as bc
from painted import PAINT_WORD

u64, u32, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p
P = bc.P


@pytest.fixture(scope="module")
def emu():
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    from build_emu import build_emulation
    lib = ctypes.CDLL(build_emulation())
    lib.emu_poly_blind.argtypes = [vp, u64, u64, u32, vp, u64, u64, ctypes.POINTER(ctypes.c_ulonglong)]
    lib.emu_split_blind.argtypes = [vp, u64, u64, u64, u32, vp, u64, u64, vp, u64, ctypes.POINTER(ctypes.c_ulonglong)]
    return lib


@pytest.mark.parametrize("h,k,batch,slack", bc.POLY_CASES)
def test_poly_blind_is_the_integer_model(emu, h, k, batch, slack):
    stride, blind_stride = h + k + slack, k + (3 if slack else 0)
    old, r = bc.poly_operands(h, k, batch)
    coeffs, blind = bc.strided(old, stride, PAINT_WORD), bc.strided(r, blind_stride, PAINT_WORD)
    blind_before, violations = blind.copy(), ctypes.c_ulonglong(0)
    assert emu.emu_poly_blind(coeffs.ctypes.data, stride, h, batch, blind.ctypes.data, blind_stride, k, ctypes.byref(violations)) == 0
    assert violations.value == 0, "an operand that must be canonical was not"
    got = coeffs.reshape(batch, stride)
    assert got[:, :h + k].tolist() == [bc.poly_blind_model(o, w, h, k) for o, w in zip(old, r)]
    assert (got[:, h + k:] == np.uint64(PAINT_WORD)).all() and np.array_equal(blind, blind_before)


def test_the_poly_cases_reach_every_borrow_and_carry():
    """the subtraction's borrow and the addition's carry in positions < k, >= h, and both in one word where k > h"""
    events = {}
    for h, k in ((h, k) for h in bc.POLY_HEIGHTS for k in bc.POLY_BLINDS):
        old, r = bc.poly_operands(h, k, 27)
        for o, w in zip(old, r):
            bc.poly_blind_model(o, w, h, k, events)
    assert sum(k > h for h in bc.POLY_HEIGHTS for k in bc.POLY_BLINDS) >= 3
    for wanted in (("low", "borrow"), ("high", "carry"), ("both", "borrow"), ("both", "carry"), ("both", "borrow and carry")):
        assert events.get(wanted, 0) > 0, wanted
    assert ("high", "borrow") not in events and ("low", "carry") not in events and not any(region == "none" for region, _ in events)


@pytest.mark.parametrize("S,L0,m,s", bc.SPLIT_CASES)
def test_split_blind_is_the_integer_model_and_recombines(emu, S, L0, m, s):
    H, b = bc.split_operands(S, L0, m, s, seed=S)
    h_stride, b_stride, out_stride = S + 3, m + 2, L0 + m + 5
    hp = bc.strided(H, h_stride, PAINT_WORD)
    bp = bc.strided([plane for per_segment in b for plane in per_segment] or [[]], b_stride, PAINT_WORD)
    out = np.full(3 * s * out_stride, PAINT_WORD, dtype=np.uint64)
    violations = ctypes.c_ulonglong(0)
    assert emu.emu_split_blind(hp.ctypes.data, h_stride, S, L0, s, bp.ctypes.data, b_stride, m, out.ctypes.data, out_stride, ctypes.byref(violations)) == 0
    assert violations.value == 0
    want = bc.split_blind_model(H, S, L0, s, b, m)
    got = out.reshape(s, 3, out_stride)
    assert got[:, :, :L0 + m].tolist() == want
    assert (got[:, :, L0 + m:] == np.uint64(PAINT_WORD)).all()
    for l, plane in enumerate(bc.recombined(want, L0, s)):
        assert plane[:S] == [v % P for v in H[l]] and not any(plane[S:]), "sum_j X^(j L0) H_j' is not H in limb plane %d" % l
    if m:
        plain = bc.split_blind_model(H, S, L0, s, [[[0] * m] * 3] * (s - 1), m)
        assert all(want[j] != plain[j] for j in range(s)), "a segment is not blinded"


def test_a_lane_outside_its_row_is_caught(emu):
    coeffs, blind, violations = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64), ctypes.c_ulonglong(0)
    assert emu.emu_poly_blind(coeffs.ctypes.data, 4, 4, 1, blind.ctypes.data, 2, 2, ctypes.byref(violations)) == -2
