"""The two blinding entries of include/bfstark_blind.h on the MI355X ("Zero-knowledge openings"): every output word against the
Python-integer models of tests/blind_cases.py on the operands that reach each borrow and carry (tests/test_blind_emulation.py checks that
they do), what the calls leave alone (tests/painted.py), every refusal of the header, the stream they keep to
(tests/blind_stream_child.py) and their export.  Exact integer arithmetic: every comparison is for equality."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import blind_cases as bc
from painted import PAINT_WORD, Arena

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_SECONDS = 120
P = bc.P


@pytest.fixture(scope="module")
def sb():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import stark_brainfuck_amd
    return stark_brainfuck_amd


# ------------------------------------------------------------------------------------------------ 1. bfsz_poly_blind
@pytest.mark.parametrize("h,k,batch,slack", bc.POLY_CASES)
def test_poly_blind_is_the_integer_model(sb, h, k, batch, slack):
    """in place in a painted arena: rows h + k + slack words apart, blinding rows k (+ 3) words apart; the slack, the guards and the
    blinding words stay as they were"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer, current_stream, synchronize
    stride, blind_stride = h + k + slack, k + (3 if slack else 0)
    old, r = bc.poly_operands(h, k, batch)
    blind = bc.strided(r, blind_stride, PAINT_WORD)
    d_blind = DeviceBuffer.from_numpy(blind)
    arena = Arena(batch=batch, stride=stride, n=h + k)
    arena.fill(0, bc.strided(old, stride, PAINT_WORD))
    _lib.check(_lib.load().bfsz_poly_blind(arena.ptr, stride, h, batch, d_blind.ptr, blind_stride, k, current_stream()))
    synchronize()
    after = arena.contained(inputs=[("blind", blind, d_blind.to_numpy())])
    assert arena.rows(after).tolist() == [bc.poly_blind_model(o, w, h, k) for o, w in zip(old, r)]


def test_poly_blind_refuses_bad_arguments_and_enqueues_nothing(sb):
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer, current_stream
    lib = _lib.load()
    d_blind = DeviceBuffer.from_numpy(np.arange(4 * 8, dtype=np.uint64))
    arena = Arena(batch=4, stride=30, n=24)
    good = [arena.ptr, 30, 16, 4, d_blind.ptr, 8, 8, current_stream()]

    def rc(at, value):
        """the call with one argument replaced -> its code, provided the refusal names the entry and the argument at fault"""
        lib.bfsg_decimate_rows(None, 0, 0, None, 0, 0, 0, None)          # (another entry's refusal: the text below is this call's own)
        assert b"bfsz_poly_blind" not in lib.bfs_last_error()
        code = lib.bfsz_poly_blind(*(good[:at] + [value] + good[at + 1:]))
        text = lib.bfs_last_error()
        return code if text.startswith(b"bfsz_poly_blind: ") and WORDS[at] in text else text
    WORDS = {0: b"null", 4: b"null", 6: b"k", 2: b"h", 1: b"stride", 5: b"blind_stride", 3: b"rows"}
    refused = {"no coefficients": rc(0, None), "no blinding words": rc(4, None), "k = 0": rc(6, 0), "h = 0": rc(2, 0), "stride < h + k": rc(1, 23),
               "blind_stride < k": rc(5, 7), "no rows": rc(3, 0), "more rows than a grid has": rc(3, 65536)}
    assert refused == {k: 6 for k in refused}
    arena.contained()             # nothing was written


# ------------------------------------------------------------------------------------------------ 2. bfsz_split_blind
@pytest.mark.parametrize("S,L0,m,s", bc.SPLIT_CASES)
def test_split_blind_is_the_integer_model_and_recombines(sb, S, L0, m, s):
    """every stride longer than its rows; sum_j X^(j L0) out_j == H on integers"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer, current_stream, synchronize
    H, b = bc.split_operands(S, L0, m, s, seed=S)
    h_stride, b_stride, out_stride = S + 3, m + 2, L0 + m + 5
    hp = bc.strided(H, h_stride, PAINT_WORD)
    bp = bc.strided([plane for per_segment in b for plane in per_segment] or [[]], b_stride, PAINT_WORD)
    d_h, d_b = DeviceBuffer.from_numpy(hp), DeviceBuffer.from_numpy(bp)
    arena = Arena(batch=3 * s, stride=out_stride, n=L0 + m)
    _lib.check(_lib.load().bfsz_split_blind(d_h.ptr, h_stride, S, L0, s, d_b.ptr, b_stride, m, arena.ptr, out_stride, current_stream()))
    synchronize()
    after = arena.contained(inputs=[("h", hp, d_h.to_numpy()), ("b", bp, d_b.to_numpy())])
    got = arena.rows(after).reshape(s, 3, L0 + m).tolist()
    assert got == bc.split_blind_model(H, S, L0, s, b, m)
    for l, plane in enumerate(bc.recombined(got, L0, s)):
        assert plane[:S] == [v % P for v in H[l]] and not any(plane[S:]), "sum_j X^(j L0) H_j' is not H in limb plane %d" % l


def test_split_blind_refuses_bad_arguments_and_enqueues_nothing(sb):
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer, current_stream
    lib = _lib.load()
    d_h, d_b = DeviceBuffer.from_numpy(np.arange(3 * 40, dtype=np.uint64)), DeviceBuffer.from_numpy(np.arange(3 * 3 * 4, dtype=np.uint64))
    arena = Arena(batch=12, stride=16, n=14)
    good = [d_h.ptr, 40, 40, 10, 4, d_b.ptr, 4, 4, arena.ptr, 16, current_stream()]          # S = 40 = 4 * 10, m = 4

    def rc(*changes):
        arguments = list(good)
        for at, value in changes:
            arguments[at] = value
        lib.bfsg_decimate_rows(None, 0, 0, None, 0, 0, 0, None)          # (another entry's refusal: the text below is this call's own)
        assert b"bfsz_split_blind" not in lib.bfs_last_error()
        code = lib.bfsz_split_blind(*arguments)
        text = lib.bfs_last_error()
        return code if text.startswith(b"bfsz_split_blind: ") and WORDS[changes[0][0]] in text else text
    WORDS = {0: b"null", 5: b"null", 8: b"null", 7: b"m <= L0", 4: b"segments", 9: b"out_stride"}
    refused = {"no polynomial": rc((0, None)), "no blinding words": rc((5, None)), "no output": rc((8, None)), "m > L0": rc((7, 11), (6, 11), (9, 30)),
               "no segments": rc((4, 0)), "17 segments": rc((4, 17)), "segments that do not cover S": rc((4, 3)), "out_stride < L0 + m": rc((9, 13))}
    assert refused == {k: 6 for k in refused}
    arena.contained()             # nothing was written


# ------------------------------------------------------------------------------------------------ 3. stream and exports
def test_the_blinding_entries_keep_to_their_stream(sb):
    """tests/blind_stream_child.py, once, in a child process under its own time limit"""
    proc = subprocess.run([sys.executable, os.path.join(HERE, "blind_stream_child.py")], capture_output=True, text=True, timeout=CHILD_SECONDS)
    lines = [json.loads(l) for l in proc.stdout.splitlines() if l.startswith("{")]
    for l in lines:
        print(json.dumps(l))
    errors = [l["error"] for l in lines if "error" in l]
    assert proc.returncode == 0 and not errors and lines and lines[-1].get("done"), "the child ended with status %s: %s\n%s" % (
        proc.returncode, errors, proc.stderr[-2000:])
    assert [l["ok"] for l in lines if "control" in l] == [True]
    by_case = {l["case"]: l for l in lines if "case" in l}
    assert len(by_case) == 2
    for name, line in by_case.items():
        assert line["kind"] == "enqueues" and line["ok"], "%s: %s" % (name, "\n".join(line["failures"]))


def test_the_library_exports_what_the_blind_header_declares(sb):
    from stark_brainfuck_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "bfstark_blind.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bfsz_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("bfsz_")}
    assert declared == exported == set(_lib.blind_exported_symbols()) == {"bfsz_poly_blind", "bfsz_split_blind"}
    assert all(getattr(lib, name).argtypes for name in declared)
    taking = set(re.findall(r"\b(bfsz_[a-z0-9_]+)\s*\([^;]*void\*\s*stream\)", text))
    import blind_stream_child as child
    assert taking == declared == {entry for case in child.blind_cases() for entry in case.entries}
    for name, count in (("bfsz_poly_blind", 8), ("bfsz_split_blind", 11)):
        arguments = re.search(name + r"\s*\(([^;]*)\)\s*;", text).group(1)
        assert len(arguments.split(",")) == len(_lib._BLIND_SIGNATURES[name][1]) == count
