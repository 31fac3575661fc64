"""The base AIR (air.py TableAir.base, the reference's base_*_constraints) and the host side of the trace checker: constraint lists
against the reference's (tests/golden/air_check.json), the generated base constraint code (csrc/air_base_generated.hpp) against the
expression graphs, and the reference's first-failure order and message format.  No GPU needed."""
import json
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "air_check.json")
TABLES = ["processor", "instruction", "memory", "input", "output"]


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _tables():
    from stark_brainfuck_amd.algebra import BaseField
    from stark_brainfuck_amd.instruction_table import InstructionTable
    from stark_brainfuck_amd.io_table import InputTable, OutputTable
    from stark_brainfuck_amd.memory_table import MemoryTable
    from stark_brainfuck_amd.processor_table import ProcessorTable
    f = BaseField.main()
    order = 1 << 32
    g = f.primitive_nth_root(order)
    return dict(zip(TABLES, [ProcessorTable(f, 4, 1, g, order), InstructionTable(f, 4, 1, g, order), MemoryTable(f, 4, 1, g, order),
                             InputTable(f, 2, g, order), OutputTable(f, 2, g, order)]))


@pytest.mark.parametrize("name", TABLES)
def test_base_constraints_match_the_reference(name):
    from stark_brainfuck_amd.algebra import BaseField, BaseFieldElement
    f = BaseField.main()
    g = golden()["constraints"][name]
    t = _tables()[name]
    bcs, tcs = t.base_boundary_constraints(), t.base_transition_constraints()
    assert [len(bcs), len(tcs)] == g["counts"]
    for cons, kind in ((bcs, "boundary_values"), (tcs, "transition_values")):
        for point, values in g[kind]:
            assert [c.evaluate([BaseFieldElement(v, f) for v in point]).value for c in cons] == values, (name, kind)


def test_the_expected_base_counts():
    """the issue's numbers: processor 5 + 6, instruction 1 + 4, memory 3 + 6, input / output none"""
    from stark_brainfuck_amd import air
    assert [[len(c) for _, c in ta.base()] for ta in air.TABLE_AIRS] == [[5, 6], [1, 4], [3, 6], [0, 0], [0, 0]]


def test_generated_base_constraint_code_matches_the_expression_graphs(tmp_path):
    """csrc/air_base_generated.hpp compiled for the host against air.evaluate at random points; the committed headers are what
    tools/gen_air.py produces from air.py today (air_generated.hpp stays byte-identical)"""
    from stark_brainfuck_amd import air
    csrc = os.path.join(ROOT, "stark_brainfuck_amd", "csrc")
    headers = [os.path.join(csrc, h) for h in ("air_generated.hpp", "air_base_generated.hpp")]
    before = [open(h).read() for h in headers]
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_air.py")], check=True, capture_output=True)
    assert [open(h).read() for h in headers] == before, "a generated AIR header is stale: run tools/gen_air.py"
    src = tmp_path / "chk.cpp"
    src.write_text(r'''
#include "%s"
#include <cstdio>
using namespace bfs;
int main() {
    u64 bc[8], bn[8], out[16]; unsigned long long v;
    auto rd = [&]() { if (scanf("%%llu", &v) != 1) return (u64)0; return (u64)v; };
    int table = (int)rd();
    for (int i = 0; i < 8; ++i) bc[i] = rd();
    for (int i = 0; i < 8; ++i) bn[i] = rd();
    int n = 0;
    if (table == 0) { airgen::air_processor_base_values(bc, bn, out); n = airgen::PROCESSOR_BASE_NUM_BOUNDARY + airgen::PROCESSOR_BASE_NUM_TRANSITION; }
    if (table == 1) { airgen::air_instruction_base_values(bc, bn, out); n = airgen::INSTRUCTION_BASE_NUM_BOUNDARY + airgen::INSTRUCTION_BASE_NUM_TRANSITION; }
    if (table == 2) { airgen::air_memory_base_values(bc, bn, out); n = airgen::MEMORY_BASE_NUM_BOUNDARY + airgen::MEMORY_BASE_NUM_TRANSITION; }
    for (int i = 0; i < n; ++i) printf("%%llu\n", (unsigned long long)out[i]);
}
''' % headers[1])
    exe = tmp_path / "chk"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), str(src)], check=True)
    rng = random.Random(17)
    P = air.P
    for ti, ta in enumerate(air.TABLE_AIRS[:3]):
        for trial in range(6):
            bc = [rng.randrange(P) for _ in range(8)]
            bn = [rng.randrange(P) for _ in range(8)]
            if trial < 3:
                bc[2] = ord(",.+-<>[]"[rng.randrange(8)])
            if trial == 5:
                bc = [rng.choice([0, 1, P - 1, 2]) for _ in range(8)]
            out = subprocess.run([str(exe)], input=" ".join(map(str, [ti] + bc + bn)), capture_output=True, text=True, check=True).stdout.split()
            cur = [air.xlift(v) for v in bc[:ta.base_width]]
            nxt = [air.xlift(v) for v in bn[:ta.base_width]]
            want = []
            for _, cons in ta.base():
                want += [air.evaluate(e, cur, nxt, [], [])[0] for e in cons]
            assert [int(v) for v in out] == want, (ta.name, trial)


def test_first_failure_order_and_message():
    """the reference loops kind, then constraint index, then row (table.py:48-110): the first failure is the lowest kind, then the
    lowest index, at that constraint's first failing row -- whatever order the entries come in"""
    from stark_brainfuck_amd.table import AirViolation, AirViolationError, first_failure_message
    assert first_failure_message([]) is None
    assert first_failure_message([AirViolation("memory", "transition", 3, 7, 0)]) is None
    vs = [AirViolation("processor", "transition", 4, 2, 5), AirViolation("processor", "transition", 1, 90, 1),
          AirViolation("processor", "terminal", 0, 127, 1)]
    assert first_failure_message(vs) == "TRNASITION constraint 1 not satisfied in row 90"
    assert first_failure_message(vs + [AirViolation("processor", "boundary", 2, 0, 1)]) == "BOUNDARY constraint 2 not satisfied in row 0"
    assert first_failure_message([AirViolation("input", "terminal", 0, 15, 1)]) == "TERMINAL constraint 0 not satisfied in row 15"
    err = AirViolationError(vs)
    assert isinstance(err, AssertionError) and err.violations == vs
    assert "processor transition constraint 1 fails on 1 row(s), first row 90" in str(err)


def test_the_check_raises_without_the_library(monkeypatch):
    """no CPU fallback: without the library the check raises like every other compute entry point"""
    from stark_brainfuck_amd import _lib
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libbfstark_hip.so")
    monkeypatch.setattr(_lib, "_lib", None)
    t = _tables()["memory"]
    t.matrix = [[0, 0, 0, 0], [1, 0, 0, 0]]
    with pytest.raises(_lib.BackendUnavailable):
        t.air_violations()
    with pytest.raises(_lib.BackendUnavailable):
        t.test()
