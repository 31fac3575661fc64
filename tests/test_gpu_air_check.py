"""The trace checker on the MI355X (bfs_air_check; Table.test / xtest / air_violations, BrainfuckStark.check_trace and check_air):
clean traces pass, the reference's verdicts on corrupted traces are reproduced (tests/golden/air_check.json), and the whole output of
the kernel equals a host recomputation through the expression graphs (air.evaluate, not the generated code) -- exhaustively on a small
trace, at wave and block edges on a trace of more than 2^20 rows."""
import ctypes
import json
import os

import numpy as np
import pytest

from test_gpu_config4 import HELLO_WORLD
from test_gpu_stark import Stream, WRAPPING_PROGRAMS

pytestmark = pytest.mark.gpu

P = (1 << 64) - (1 << 32) + 1
NONE = (2 ** 64 - 1, 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "air_check.json")
TABLES = ["processor", "instruction", "memory", "input", "output"]
CHALLENGES = [((7 * i + 3) << 40 | 12345, (i + 1) << 35, 99 + i) for i in range(11)]
INITIALS = [(1 << 50 | 77, 5, 6), (3 << 45 | 11, 7, 8)]

CLEAN = [(HELLO_WORLD, ""), (",+.,-.", "ab"), (",[.,]", "hello\x00"), ("+[-]>++<", ""), ("++[>+++<-]>.", "")] + \
        [(code, "") for code in WRAPPING_PROGRAMS[:4]]


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _trace(code, inputs=""):
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    from stark_brainfuck_amd.vm import VirtualMachine
    program = VirtualMachine.compile(code)
    matrices = VirtualMachine.simulate(program, input_data=list(inputs), max_cycles=5000)
    inp = [chr(int(v)) for v in matrices[3].values.reshape(-1)]
    out = [chr(int(v) % 256) for v in matrices[4].values.reshape(-1)]
    stark = BrainfuckStark(len(matrices[0]), len(matrices[1]), program, inp, out)
    return stark, program, matrices


def _tables(stark, matrices):
    """the stark's tables holding (fresh references to) the matrices, keyed by name"""
    pm, mm, im, inm, om = matrices
    t = dict(zip(TABLES, stark.tables))
    for name, m in zip(["processor", "memory", "instruction", "input", "output"], matrices):
        t[name].matrix = m
    return t


def _extended(stark, matrices, challenges=CHALLENGES, initials=INITIALS):
    t = _tables(stark, matrices)
    for table in stark.tables:
        table.pad()
    for table in stark.tables:
        table.extend(challenges, initials)
    return t, stark.get_terminals()


def _first(violations):
    order = {"boundary": 0, "transition": 1, "terminal": 2}
    if not violations:
        return "pass"
    v = min(violations, key=lambda v: (order[v.kind], v.index))
    return [v.kind, v.index, v.first_row]


def _check_raw(table, extended, d_base, d_ext, rows, ld, challenges=None, terminals=None, params=None):
    """every entry of bfs_air_check's output as (first_row, count)"""
    from stark_brainfuck_amd import _lib, air
    from stark_brainfuck_amd.device import current_stream
    u64 = ctypes.c_uint64
    ta = air.TABLE_AIRS[table]
    nq = sum(len(c) for _, c in (ta.all() if extended else ta.base()))
    out = (_lib.AirViolation * max(nq, 1))()
    ch = (u64 * 33)(*[v for c in challenges for v in c]) if challenges else None
    tm = (u64 * 15)(*[v for c in terminals for v in c]) if terminals else None
    pr = (u64 * 3)(*params) if params else None
    _lib.check(_lib.load().bfs_air_check(table, extended, d_base, d_ext, rows, ld, ch, tm, pr, out, current_stream()))
    return [(int(o.first_row), int(o.count)) for o in out[:nq]]


class HostAir:
    """per row and constraint, "is the value non-zero and does the constraint apply here", from the expression graphs"""

    def __init__(self, ta, base, ext, extended, challenges=(), terminals=(), params=()):
        from stark_brainfuck_amd import air
        self.air, self.ta, self.extended = air, ta, extended
        self.base, self.ext = base, ext               # base: (width, rows) ints; ext: list of (3, rows) per extension column
        self.ch, self.tm, self.pr = challenges, terminals, params
        self.kinds = ta.all() if extended else ta.base()
        self.rows = base.shape[1]
        self.flags = [self.row_flags(r) for r in range(self.rows)]

    def point(self, r):
        air = self.air
        pt = [air.xlift(int(v)) for v in self.base[:, r]]
        if self.extended:
            pt += [tuple(int(x) % P for x in col[:, r]) for col in self.ext]
        return pt

    def row_flags(self, r):
        cur, nxt = self.point(r), self.point(min(r + 1, self.rows - 1))
        flags, memo = [], {}
        for kind, cons in self.kinds:
            applies = {"boundary": r == 0, "transition": r + 1 < self.rows, "terminal": r + 1 == self.rows}[kind]
            for e in cons:
                flags.append(applies and any(self.air.evaluate(e, cur, nxt, self.ch, self.tm, self.pr, memo)))
        return flags

    def refresh(self, r):
        for k in (r - 1, r):
            if 0 <= k < self.rows:
                self.flags[k] = self.row_flags(k)

    def expected(self):
        nq = sum(len(c) for _, c in self.kinds)
        out = []
        for q in range(nq):
            failing = [r for r in range(self.rows) if self.flags[r][q]]
            out.append((failing[0], len(failing)) if failing else NONE)
        return out


# ---- 1. clean traces ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code,inputs", CLEAN)
def test_clean_traces_pass(code, inputs):
    stark, program, matrices = _trace(code, inputs)
    t = _tables(stark, matrices)
    for name in TABLES:
        t[name].test()                                        # unpadded
    stark, program, matrices = _trace(code, inputs)
    t, terminals = _extended(stark, matrices)
    for name in TABLES:
        t[name].xtest(CHALLENGES, terminals)
    stark, program, matrices = _trace(code, inputs)
    before = [m.values.copy() for m in matrices]
    assert stark.check_trace(*matrices) == []
    assert stark.check_trace(*matrices, challenges=CHALLENGES, initials=INITIALS) == []
    assert all(np.array_equal(b, m.values) and len(m) == b.shape[0] for b, m in zip(before, matrices))      # the caller's matrices


# ---- 2. the reference's verdicts --------------------------------------------------------------------------------------------------------
def test_the_reference_verdicts_of_test():
    from stark_brainfuck_amd.table import first_failure_message
    for entry in golden()["programs"]:
        stark, program, matrices = _trace(entry["code"], entry["input"])
        t = _tables(stark, matrices)
        assert {n: len(t[n].matrix) for n in TABLES} == entry["lengths"]
        for name in TABLES:
            assert _first(t[name].air_violations()) == entry["unpadded"][name], (entry["code"], name)
        stark, program, matrices = _trace(entry["code"], entry["input"])
        t = _tables(stark, matrices)
        for name in TABLES:
            t[name].pad()
            assert _first(t[name].air_violations()) == entry["padded"][name], (entry["code"], name, "padded")
        for case in entry["corruptions"]:
            stark, program, matrices = _trace(entry["code"], entry["input"])
            t = _tables(stark, matrices)
            arr = t[case["table"]].base_array()
            arr[case["column"], case["row"]] = (int(arr[case["column"], case["row"]]) + case["add"]) % P
            got = t[case["table"]].air_violations()
            assert _first(got) == case["verdict"], (entry["code"], case)
            if case["verdict"] == "pass":
                t[case["table"]].test()
            else:
                with pytest.raises(AssertionError) as e:
                    t[case["table"]].test()
                assert str(e.value) == first_failure_message(got)
                assert ("constraint %d not satisfied in row %d" % (case["verdict"][1], case["verdict"][2])) in str(e.value)


def test_the_reference_verdicts_of_xtest():
    g = golden()["xtest"]
    challenges = [tuple(c) for c in g["challenges"]]
    initials = [tuple(c) for c in g["initials"]]
    for entry in g["programs"]:
        stark, program, matrices = _trace(entry["code"], entry["input"])
        t, terminals = _extended(stark, matrices, challenges, initials)
        assert [list(x) for x in terminals] == entry["terminals"]
        for name in TABLES:
            got = _first(t[name].air_violations(challenges, terminals)) if t[name].length else "pass"
            assert got == entry["clean"][name], (entry["code"], name)
        for case in entry["corruptions"]:
            stark, program, matrices = _trace(entry["code"], entry["input"])
            t, terminals = _extended(stark, matrices, challenges, initials)
            table = t[case["table"]]
            col, row = case["column"], case["row"]
            if col < table.base_width:
                arr = table.base_array()
                arr[col, row] = (int(arr[col, row]) + case["add"]) % P
            else:
                ext = table.ext_columns[col - table.base_width]
                ext[0, row] = (int(ext[0, row]) + case["add"]) % P
            assert _first(table.air_violations(challenges, terminals)) == case["verdict"], (entry["code"], case)
            with pytest.raises(AssertionError):
                table.xtest(challenges, terminals)


# ---- 3. exhaustive on a small trace -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extended", [False, True])
def test_every_cell_of_a_small_trace(extended):
    """every cell of every table corrupted in turn: the whole output equals the host recomputation"""
    from stark_brainfuck_amd import air
    from stark_brainfuck_amd.device import DeviceBuffer
    stark, program, matrices = _trace(",+[>++<-].", "\x03")
    if extended:
        t, terminals = _extended(stark, matrices)
    else:
        t, terminals = _tables(stark, matrices), None
    for name in TABLES:
        table = t[name]
        ta = table.air
        base = np.array(table.base_array(), dtype=np.uint64, copy=True)
        rows = base.shape[1]
        if rows == 0 or not sum(len(c) for _, c in (ta.all() if extended else ta.base())):
            continue
        ext = [np.array(c, dtype=np.uint64, copy=True) for c in table.ext_columns] if extended else []
        params = table.air_params(CHALLENGES) if extended else []
        host = HostAir(ta, base.astype(object), [e.astype(object) for e in ext], extended, CHALLENGES,
                       [tuple(x) for x in terminals] if extended else (), params)
        d_base = DeviceBuffer.from_numpy(base.reshape(-1))
        d_ext = DeviceBuffer.from_numpy(np.concatenate(ext, axis=0).reshape(-1)) if ext else None
        run = lambda: _check_raw(table.table_index, int(extended), d_base.ptr, d_ext.ptr if d_ext else None, rows, rows,
                                 CHALLENGES if extended else None, terminals if extended else None, params[0] if params else None)
        assert run() == host.expected(), (name, "clean")
        cells = [("b", c) for c in range(base.shape[0])] + [("x", (k, l)) for k in range(len(ext)) for l in range(3)]
        for kind, c in cells:
            for r in range(rows):
                if kind == "b":
                    old = base[c, r]
                    base[c, r] = (int(old) + 1) % P
                    d_base = DeviceBuffer.from_numpy(base.reshape(-1))
                    host.base = base.astype(object)
                else:
                    k, l = c
                    old = ext[k][l, r]
                    ext[k][l, r] = (int(old) + 1) % P
                    d_ext = DeviceBuffer.from_numpy(np.concatenate(ext, axis=0).reshape(-1))
                    host.ext = [e.astype(object) for e in ext]
                host.refresh(r)
                assert run() == host.expected(), (name, kind, c, r)
                if kind == "b":
                    base[c, r] = old
                    d_base = DeviceBuffer.from_numpy(base.reshape(-1))
                    host.base = base.astype(object)
                else:
                    ext[c[0]][c[1], r] = old
                    d_ext = DeviceBuffer.from_numpy(np.concatenate(ext, axis=0).reshape(-1))
                    host.ext = [e.astype(object) for e in ext]
                host.refresh(r)
        d_base = DeviceBuffer.from_numpy(base.reshape(-1))
        d_ext = DeviceBuffer.from_numpy(np.concatenate(ext, axis=0).reshape(-1)) if ext else None
        assert run() == host.expected(), (name, "restored")


def test_row_counts_and_arguments():
    """rows == 0 evaluates nothing; any row count; bad arguments are errors, violations are not"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer
    assert _check_raw(2, 0, None, None, 0, 0) == [NONE] * 9
    assert _check_raw(0, 1, None, None, 0, 0, CHALLENGES, [(0, 0, 0)] * 5) == [NONE] * 21
    one = DeviceBuffer.from_numpy(np.array([5, 0, 0, 1], dtype=np.uint64))            # one memory row: boundary 0 fails (clk = 5)
    assert _check_raw(2, 0, one.ptr, None, 1, 1) == [(0, 1)] + [NONE] * 8
    with pytest.raises(RuntimeError):
        _check_raw(2, 0, one.ptr, None, 2, 1)                                            # ld < rows
    out = (_lib.AirViolation * 32)()
    assert _lib.load().bfs_air_check(7, 0, one.ptr, None, 1, 1, None, None, None, out, None) != 0           # no table 7
    assert _lib.load().bfs_air_check(0, 2, one.ptr, None, 1, 1, None, None, None, out, None) != 0           # extended is 0 or 1
    counts = (ctypes.c_int * 2)()
    for table, want in enumerate([(5, 6), (1, 4), (3, 6), (0, 0), (0, 0)]):
        _lib.check(_lib.load().bfs_air_base_counts(table, counts))
        assert tuple(counts) == want


# ---- 4. large traces --------------------------------------------------------------------------------------------------------------------
def _big_nested():
    return "+" * 350 + "[>" + "+" * 350 + "[>++++<-]<-]+++."


def test_large_trace_wave_and_block_edges():
    """a processor trace of more than 2^20 rows: clean, then single cells at row 0, the last row, rows 63 / 64 and 255 / 256 (wave and
    block edges) and the last row of a later block; each output equals the host evaluation of the rows that read the cell, every other
    entry {UINT64_MAX, 0}.  One strided case: ld > rows with non-zero garbage in the gap."""
    from stark_brainfuck_amd import _lib, air
    from stark_brainfuck_amd.device import DeviceBuffer, current_stream
    from stark_brainfuck_amd.vm import VirtualMachine
    program = VirtualMachine.compile(_big_nested())
    pm = VirtualMachine.simulate(program, input_data=[], max_cycles=1 << 22)[0]
    base = np.ascontiguousarray(pm.values[:, :7].T)
    rows = base.shape[1]
    assert rows >= 1 << 20
    ta = air.TABLE_AIRS[0]
    lib, stream = _lib.load(), current_stream()
    d = DeviceBuffer.from_numpy(base.reshape(-1))
    assert _check_raw(0, 0, d.ptr, None, rows, rows) == [NONE] * 11

    def host_rows(cells, r):
        h = [[False] * 11 for _ in range(rows)]
        for k in (r - 1, r):
            if 0 <= k < rows:
                cur = [air.xlift(int(v)) for v in cells[:, k]]
                nxt = [air.xlift(int(v)) for v in cells[:, min(k + 1, rows - 1)]]
                q = 0
                for kind, cons in ta.base():
                    for e in cons:
                        applies = k == 0 if kind == "boundary" else k + 1 < rows
                        h[k][q] = applies and air.evaluate(e, cur, nxt, [], [])[0] != 0
                        q += 1
        out = []
        for q in range(11):
            failing = [k for k in (r - 1, r) if 0 <= k < rows and h[k][q]]
            out.append((failing[0], len(failing)) if failing else NONE)
        return out
    for r in (0, rows - 1, 63, 64, 255, 256, 1 << 19 | 255):
        for c, add in ((0, 1), (5, P - 1), (2, 1)):
            old = int(base[c, r])
            patch = np.array([(old + add) % P], dtype=np.uint64)
            _lib.check(lib.bfs_memcpy_h2d(d.ptr + 8 * (c * rows + r), patch.ctypes.data, 8, stream))
            base[c, r] = patch[0]
            got = _check_raw(0, 0, d.ptr, None, rows, rows)
            assert got == host_rows(base, r), (r, c)
            base[c, r] = old
            patch[0] = old
            _lib.check(lib.bfs_memcpy_h2d(d.ptr + 8 * (c * rows + r), patch.ctypes.data, 8, stream))
    assert _check_raw(0, 0, d.ptr, None, rows, rows) == [NONE] * 11
    # strided: the columns inside a wider buffer, garbage in the gap that must not be read
    ld = rows + 1000
    wide = np.full((7, ld), 12345, dtype=np.uint64)
    wide[:, :rows] = base
    r = 64
    wide[4, r] = (int(wide[4, r]) + 1) % P
    dw = DeviceBuffer.from_numpy(wide.reshape(-1))
    assert _check_raw(0, 0, dw.ptr, None, rows, ld) == host_rows(wide[:, :rows], r)


# ---- 5. check_air in prove() ------------------------------------------------------------------------------------------------------------
def _hello(monkeypatch, tag):
    from stark_brainfuck_amd import brainfuck_stark, salted_merkle, table
    stark, program, matrices = _trace(HELLO_WORLD)
    stream = Stream(tag)
    for mod in (brainfuck_stark, salted_merkle, table):
        monkeypatch.setattr(mod, "urandom", stream)
    return stark, program, matrices


def test_check_air_gives_the_same_proof(monkeypatch):
    stark, program, matrices = _hello(monkeypatch, b"air-check")
    proof = stark.prove(program, *matrices)
    stark, program, matrices = _hello(monkeypatch, b"air-check")
    stark.check_air = True
    assert stark.prove(program, *matrices) == proof


def test_check_air_stops_a_corrupted_trace_before_fri(monkeypatch):
    from stark_brainfuck_amd import AirViolationError
    from stark_brainfuck_amd.fri import Fri
    stark, program, matrices = _hello(monkeypatch, b"air-check-bad")
    row = len(matrices[0]) // 2
    matrices[0].values[row, 6] = (int(matrices[0].values[row, 6]) + 1) % P      # memory value inverse
    stark.check_air = True

    def no_fri(*args, **kwargs):
        raise RuntimeError("FRI reached")
    monkeypatch.setattr(Fri, "prove", no_fri)
    with pytest.raises(AirViolationError) as e:
        stark.prove(program, *matrices)
    vs = e.value.violations
    assert vs and all(v.table == "processor" for v in vs)
    assert ("processor", "transition", 5, row) in [(v.table, v.kind, v.index, v.first_row) for v in vs]
    assert "processor transition constraint 5" in str(e.value)
    monkeypatch.undo()
    stark, program, _ = _hello(monkeypatch, b"air-check-bad")
    proof = stark.prove(program, *matrices)                                    # the switch off: a proof, which verify() rejects
    assert stark.verify(proof) is False


# ---- 6. cross-table checks --------------------------------------------------------------------------------------------------------------
def test_check_trace_reports_an_output_terminal_mismatch():
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    stark, program, matrices = _trace(",+.,-.", "ab")
    wrong = BrainfuckStark(stark.running_time, stark.memory_length, program, stark.input_symbols, ["x", "y"])
    got = wrong.check_trace(*matrices, challenges=CHALLENGES, initials=INITIALS)
    assert [(v.table, v.kind, v.index) for v in got] == [("processor", "evaluation", 1)]


def test_check_trace_reports_a_permutation_mismatch():
    stark_a, program_a, ma = _trace("++[>+++<-]>.")
    stark_b, program_b, mb = _trace("+++[>++<-]>.")
    mixed = (ma[0], ma[1], mb[2], ma[3], ma[4])
    got = stark_a.check_trace(*mixed, challenges=CHALLENGES, initials=INITIALS)
    assert ("processor", "permutation", 0) in [(v.table, v.kind, v.index) for v in got]
    assert not [v for v in got if v.kind in ("boundary", "transition", "terminal")]
