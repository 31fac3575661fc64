"""The REJECTING side of the STARK on the MI355X: proofs of false traces are written (the prover does not check its witness) and both
verifier routes -- csrc/verifier.cpp and _verify_stream / Fri.verify in Python -- refuse them.

  a. the reference's own false traces (tests/golden/soundness.json, gen_soundness_golden.py): one cell of the trace of `+.` changed.  Both
     prover paths write the reference's bytes -- the quotient kernels on numerators that do NOT vanish on the trace domain, which no
     honest fixture exercises -- and both routes end as the reference's verify did;
  b. a fixed list of one-cell changes over all five matrices of `,+[>++<-].`: flagged by check_trace, the same bytes from both prover
     paths, refused by both routes alike, and the measured reason: the combination codeword's degree exceeds max_degree.  A separate
     test asserts that the list violates every base constraint of every table that has any;
  c. lies in EXTENSION columns (a limb changed in HBM behind the honest extension, Python stage path);
  d. coherent false executions from a small dishonest simulator written here.

`outcome` (tests/soundness_cases.py) computes a verdict inside its `try`; every assertion here is made on the returned value."""
import ctypes
import hashlib

import numpy as np
import pytest

import pointwise_check as pc
from soundness_cases import ACCEPTED, MATRICES, P, outcome, recorded, soundness
from test_gpu_air_check import CHALLENGES, INITIALS
from test_gpu_prover_pointwise import _quotients, _read_back
from test_gpu_stark import Stream

pytestmark = pytest.mark.gpu

TABLE_ORDER = ["processor", "instruction", "memory", "input", "output"]          # BrainfuckStark.tables


def _trace(code, inputs=""):
    """(program, claim arguments, {name: matrix}) of an honest run"""
    from stark_brainfuck_amd.vm import VirtualMachine
    program = VirtualMachine.compile(code)
    running_time, input_symbols, output_symbols = VirtualMachine.run(program, input_data=list(inputs))
    matrices = dict(zip(MATRICES, VirtualMachine.simulate(program, input_data=list(input_symbols))))
    return program, (running_time, len(matrices["memory"]), program, input_symbols, output_symbols), matrices


def _wrap(values, width):
    """a trace matrix over an array of our own"""
    from stark_brainfuck_amd.vm import LazyTraceMatrix, VirtualMachine
    return LazyTraceMatrix(np.ascontiguousarray(np.array(values, dtype=np.uint64).reshape(-1, width)), VirtualMachine.field)


def _prove(monkeypatch, tag, claim, program, matrices, **attributes):
    """one proof from the fixed stream `tag`; attributes are set on the prover first -> (prover, proof, urandom bytes drawn)"""
    from stark_brainfuck_amd import brainfuck_stark, salted_merkle, table
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    stream = Stream(tag)
    for mod in (brainfuck_stark, salted_merkle, table):
        monkeypatch.setattr(mod, "urandom", stream)
    monkeypatch.delenv("DEBUG", raising=False)
    monkeypatch.delenv("BFS_DEBUG", raising=False)
    stark = BrainfuckStark(*claim)
    for key, value in attributes.items():
        setattr(stark, key, value)
    proof = stark.prove(program, *(matrices[k] for k in MATRICES))
    return stark, proof, stream.pos


def _flagged(claim, matrices):
    """what check_trace says about the matrices: the base AIR as given, the full AIR on padded, extended copies, the cross-table terminals"""
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    return BrainfuckStark(*claim).check_trace(*(matrices[k] for k in MATRICES), challenges=CHALLENGES, initials=INITIALS)


def _refused_alike(claim, proof):
    """both routes' outcome of verify; they must be equal and not an acceptance"""
    native, python = outcome(claim, proof, True), outcome(claim, proof, False)
    assert native == python, (native, python)
    assert native != ACCEPTED
    return native


def _bump(matrix, row, column, add):
    v = matrix.values
    v[row, column] = (int(v[row, column]) + add) % P


# ---- a. the reference's false traces -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", soundness()["false_traces"]["cases"], ids=lambda c: c["tag"])
def test_false_traces_get_the_reference_bytes_and_the_reference_verdict(case, monkeypatch):
    g = soundness()["false_traces"]
    program, claim, matrices = _trace(g["program"])
    assert {k: [m.values.shape[0], m.values.shape[1] if m.values.shape[0] else 0] for k, m in matrices.items()} == case["shapes"]
    assert int(matrices[case["matrix"]].values[case["row"], case["column"]]) == case["honest_value"]
    _bump(matrices[case["matrix"]], case["row"], case["column"], case["add"])
    claim = claim[:4] + (list(case["claimed_output"]),)
    assert (claim[0], claim[1]) == (case["running_time"], case["memory_length"])
    tag = ("soundness-" + case["tag"]).encode()
    proofs = []
    for path, attributes in (("native stage driver", {}), ("keep_intermediates", {"keep_intermediates": True})):
        stark, proof, drawn = _prove(monkeypatch, tag, claim, program, matrices, **attributes)
        assert stark.fri.domain.length == case["fri_domain_length"] and stark.max_degree == case["max_degree"]
        assert drawn == case["urandom_bytes"], path
        assert (len(proof), hashlib.sha256(proof).hexdigest()) == (case["proof_len"], case["proof_sha256"]), path
        proofs.append(proof)
    want = recorded(case["outcome"])
    assert want != ACCEPTED                                   # (what the fixture is for)
    for native in (True, False):
        assert outcome(claim, proofs[0], native) == want, "native" if native else "python"


# ---- b. one cell of `,+[>++<-].` ------------------------------------------------------------------------------------------------------------
CELL_PROGRAM, CELL_INPUT = ",+[>++<-].", "\x03"          # 29 cycles; processor 29 -> 32 rows, memory 49 -> 64, instruction 41 -> 64, one symbol in, one out
# (matrix, row, column, add).  Rows: first, second, middle, the last two, and -- rows past the end of a matrix -- PADDING rows: the matrix
# is handed to prove() with that many of the padding rows the prover itself would have added (processor and instruction matrix together:
# prove() asserts their lengths against each other), the cell changed in one of them.  Columns: processor clk ip ci ni mp mv inv,
# memory clk mp mv dummy, instruction ip ci ni.  Some cells break no BASE constraint (a next instruction, a memory value between two
# consecutive cycles, the inverse in the last row): only the full AIR on the padded table or a permutation argument sees those.
CELL_CASES = [
    ("processor", 0, 0, 1), ("processor", 0, 1, 1), ("processor", 0, 2, 1), ("processor", 0, 3, 1), ("processor", 0, 4, 1),
    ("processor", 0, 5, 1), ("processor", 0, 6, 1), ("processor", 1, 5, P - 1), ("processor", 2, 5, 1), ("processor", 2, 2, 1),
    ("processor", 14, 3, 1), ("processor", 14, 6, 5), ("processor", 15, 0, 1), ("processor", 15, 4, P - 1), ("processor", 27, 5, 1),
    ("processor", 28, 0, 1), ("processor", 28, 4, 1), ("processor", 28, 5, 1), ("processor", 28, 6, 1),
    ("processor", 29, 0, 1), ("processor", 31, 0, 1),
    ("memory", 0, 0, 1), ("memory", 0, 1, 1), ("memory", 0, 2, 1), ("memory", 1, 3, 5), ("memory", 1, 2, 1), ("memory", 24, 1, 1),
    ("memory", 24, 2, P - 1), ("memory", 24, 3, 1), ("memory", 25, 3, 1), ("memory", 47, 0, 1), ("memory", 48, 1, 1), ("memory", 48, 2, 1),
    ("memory", 49, 1, 1), ("memory", 63, 0, 1),
    ("instruction", 0, 0, 1), ("instruction", 0, 1, 1), ("instruction", 0, 2, 1), ("instruction", 2, 0, 1), ("instruction", 2, 1, 1),
    ("instruction", 20, 0, 1), ("instruction", 21, 2, 5), ("instruction", 39, 1, 1), ("instruction", 40, 0, 1), ("instruction", 40, 2, 1),
    ("instruction", 41, 1, 1),
    ("input", 0, 0, 1), ("output", 0, 0, 1),
]
assert len(CELL_CASES) <= 48 and len(set(CELL_CASES)) == len(CELL_CASES)
POINTWISE_CASES = {("processor", 2, 5, 1), ("memory", 24, 1, 1), ("instruction", 2, 0, 1), ("input", 0, 0, 1), ("output", 0, 0, 1)}
# base constraints that no one-cell change of this trace can violate: (table, kind, index) -> why.  None are needed.
UNREACHABLE_BASE_CONSTRAINTS = {}


def _padded_rows(claim, matrices, name, count):
    """matrix `name` with the first `count` of the padding rows Table.pad would add"""
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    table = BrainfuckStark(*claim).tables[TABLE_ORDER.index(name)]
    table.matrix = matrices[name]
    table.pad()
    rows = len(matrices[name])
    padded = np.array(table.base_array(), dtype=np.uint64).T
    assert padded.shape[0] == table.height >= rows + count and np.array_equal(padded[:rows], matrices[name].values[:, :padded.shape[1]])
    return _wrap(padded[:rows + count], padded.shape[1])


def _cell_case(case):
    """(program, claim, matrices) with the cell of `case` changed"""
    name, row, column, add = case
    program, claim, matrices = _trace(CELL_PROGRAM, CELL_INPUT)
    extra = row + 1 - len(matrices[name])
    if extra > 0:
        for other in (("processor", "instruction") if name in ("processor", "instruction") else (name,)):
            matrices[other] = _padded_rows(claim, matrices, other, extra)
    assert 0 <= row < matrices[name].values.shape[0] and 0 <= column < matrices[name].values.shape[1]
    _bump(matrices[name], row, column, add)
    return program, claim, matrices


@pytest.mark.parametrize("case", CELL_CASES, ids=lambda c: "%s-r%d-c%d" % c[:3])
def test_one_changed_cell_is_proven_and_refused(case, monkeypatch):
    program, claim, matrices = _cell_case(case)
    violations = _flagged(claim, matrices)                                          # 1. not vacuous: the trace is false
    assert violations, case
    tag = ("soundness-cell-%s-%d-%d" % case[:3]).encode()
    _, proof, drawn = _prove(monkeypatch, tag, claim, program, matrices)             # 2. both prover paths, the same bytes
    stark, kept, drawn_kept = _prove(monkeypatch, tag, claim, program, matrices, keep_intermediates=True)
    assert proof == kept and drawn == drawn_kept
    verdict = _refused_alike(claim, proof)                                          # 3. refused, by both routes alike
    combination = stark._last["combination"].to_numpy()                             # 4. why: the combination is no low-degree codeword
    degree = pc.degree(combination, stark.fri.domain.omega.value)
    print("%s: %s; combination degree %d, max_degree %d; %s" % (case, verdict, degree, stark.max_degree,
                                                                  ["%s %s %d" % (v.table, v.kind, v.index) for v in violations]))
    assert degree > stark.max_degree, (degree, stark.max_degree)
    if case in POINTWISE_CASES:
        # the kernels computed the quotients of the FALSE trace correctly: every quotient and the combination on sampled rows against
        # Python integers over the expression graphs (the degree half of the checker is what fails here, by design)
        base, ext, randomizer, spec = _read_back(stark)
        rows = pc.sample_rows(spec.n, spec.unit_distances(), count=32, seed=spec.n)
        checker = pc.Checker(spec, base, ext, randomizer, rows)
        failures = [f for f in checker.inputs(degrees=False)]
        too_high = 0
        for q, load in _quotients(stark):
            codeword = load()
            failures += checker.quotient(q, codeword, check_degree=False)
            too_high += pc.degree(codeword, spec.omega) > max(spec.quotient_degree_bounds[q], -1)
        failures += checker.combination(combination, check_degree=False)
        assert not failures, "\n".join("%s: %s" % f for f in failures[:20])
        assert too_high >= 1, "no quotient exceeds its degree bound"


def test_a_false_trace_with_a_low_degree_combination_is_refused_by_the_program_evaluation(monkeypatch):
    """Not every false trace breaks the AIR.  The address in the first padding row of the instruction table raised by one (12 -> 13)
    is a step the instruction table's constraints allow -- it reads as one more row of the program listing -- so every quotient is a
    polynomial and the combination codeword keeps its degree bound: FRI has nothing to object to.  What refuses the proof is the
    last check of verify(), the program evaluation terminal against the program of the claim (measured on the MI355X: combination degree
    1023 = max_degree, check_trace names the instruction table's evaluation terminal and nothing else, both routes say False)."""
    case = ("instruction", 41, 0, 1)
    program, claim, matrices = _cell_case(case)
    violations = _flagged(claim, matrices)
    assert [(v.table, v.kind, v.index) for v in violations] == [("instruction", "evaluation", 2)]
    tag = ("soundness-cell-%s-%d-%d" % case[:3]).encode()
    _, proof, _ = _prove(monkeypatch, tag, claim, program, matrices)
    stark, kept, _ = _prove(monkeypatch, tag, claim, program, matrices, keep_intermediates=True)
    assert proof == kept
    assert pc.degree(stark._last["combination"].to_numpy(), stark.fri.domain.omega.value) <= stark.max_degree
    assert _refused_alike(claim, proof) == ("value", False)


def test_cell_cases_violate_every_base_constraint():
    """the list above is wide enough: over its cases, air_violations (bfs_air_check, base AIR on the matrices as handed over) names
    every base constraint that bfs_air_base_counts counts, for every table that has any, except those listed as unreachable -- at
    most two, each with its reason"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    assert len(UNREACHABLE_BASE_CONSTRAINTS) <= 2 and all(UNREACHABLE_BASE_CONSTRAINTS.values())
    every = set()
    counts = (ctypes.c_int * 2)()
    for index, name in enumerate(TABLE_ORDER):
        _lib.check(_lib.load().bfs_air_base_counts(index, counts))
        every |= {(name, "boundary", i) for i in range(counts[0])} | {(name, "transition", i) for i in range(counts[1])}
    assert len(every) == 11 + 5 + 9                                                  # (processor, instruction, memory; the IO tables have none)
    seen = set()
    for case in CELL_CASES:
        program, claim, matrices = _cell_case(case)
        got = BrainfuckStark(*claim).check_trace(*(matrices[k] for k in MATRICES))
        assert all(v.table == case[0] for v in got), (case, got)
        seen |= {(v.table, v.kind, v.index) for v in got}
    assert seen <= every
    assert not seen & set(UNREACHABLE_BASE_CONSTRAINTS), "listed as unreachable, but violated"
    assert every - seen == set(UNREACHABLE_BASE_CONSTRAINTS), sorted(every - seen)


# ---- c. lies in extension columns ------------------------------------------------------------------------------------------------------
EXT_PROGRAM, EXT_INPUT = ",.,.,.", "abc"          # heights 8, 16, 8, 4, 4 (three symbols in, three out: the IO tables have a padding row)
EXT_CASES = [(name, where) for name in TABLE_ORDER for where in ("first", "middle", "last")]


@pytest.mark.parametrize("name,where", EXT_CASES)
def test_a_lie_in_an_extension_column_is_refused(name, where, monkeypatch):
    """after the honest extension (extend_tables_device, Python stage path) one limb of one row of one extension column of table `name`
    is changed in HBM: the commitment, the quotients and FRI are all made over the lie.  The full AIR on the extended tables (bfs_air_check
    on the very buffers the prover goes on with, against the terminals the prover sends) flags it, and both routes refuse the proof."""
    from stark_brainfuck_amd import _lib, brainfuck_stark
    from stark_brainfuck_amd.device import current_stream, synchronize
    program, claim, matrices = _trace(EXT_PROGRAM, EXT_INPUT)
    honest = brainfuck_stark.extend_tables_device
    seen = {}

    def lying(tables, challenges, initials, prepared=None):
        honest(tables, challenges, initials, prepared=prepared)
        table = tables[TABLE_ORDER.index(name)]
        height, width = table.height, table.full_width - table.base_width
        assert height >= 4 and width >= 1 and table.length >= 3
        row = {"first": 0, "middle": table.length // 2, "last": height - 1}[where]
        column, limb = row % width, row % 3
        at = 3 * column * height + limb * height + row                  # column-major: three limb planes of `height` words per column
        assert 0 <= row < height and at < table._ext_device.count == 3 * width * height
        word = np.array([(int(table._ext_device.to_numpy(1, offset=at)[0]) + 1) % P], dtype=np.uint64)
        _lib.check(_lib.load().bfs_memcpy_h2d(table._ext_device.ptr + 8 * at, word.ctypes.data, 8, current_stream()))
        synchronize(current_stream())
        terminals = [tables[0].instruction_permutation_terminal, tables[0].memory_permutation_terminal, tables[0].input_evaluation_terminal,
                     tables[0].output_evaluation_terminal, tables[1].evaluation_terminal]
        seen["violations"] = [v for t in tables if t.length for v in t.air_violations(challenges, terminals)]
        seen["cell"] = (row, column, limb)
    monkeypatch.setattr(brainfuck_stark, "extend_tables_device", lying)
    stark, proof, _ = _prove(monkeypatch, ("soundness-ext-%s-%s" % (name, where)).encode(), claim, program, matrices, native_stages=False)
    assert stark.fri.domain.length == 1024
    monkeypatch.setattr(brainfuck_stark, "extend_tables_device", honest)
    print(name, where, seen["cell"], ["%s %s %d row %s" % (v.table, v.kind, v.index, v.first_row) for v in seen["violations"]])
    assert seen["violations"] and all(v.table == name for v in seen["violations"]), seen
    _refused_alike(claim, proof)
    # the same prover with the honest extension writes a proof that both routes accept: the refusal is the lie's
    _, proof, _ = _prove(monkeypatch, ("soundness-ext-%s-%s" % (name, where)).encode(), claim, program, matrices, native_stages=False)
    assert outcome(claim, proof, True) == outcome(claim, proof, False) == ACCEPTED


# ---- d. coherent false executions -------------------------------------------------------------------------------------------------------
def _dishonest_run(code, inputs="", enter_every_loop=False):
    """A Brainfuck machine that records the five matrices -- and, with enter_every_loop, steps INTO a loop whose cell is zero, writing
    1 into the inverse column of that row (a zero has no inverse to store).  Everything else it does by the rules, so the trace is a
    coherent execution of a machine that is not the Brainfuck machine.  -> {name: rows}"""
    from stark_brainfuck_amd.vm import VirtualMachine
    words = [w.value for w in VirtualMachine.compile(code)]
    size = len(words)
    cells, fed = {}, list(inputs)
    clk = ip = mp = 0
    processor, executed, read, written = [], [], [], []
    while True:
        ci = words[ip] if ip < size else 0
        ni = words[ip + 1] if ip + 1 < size else 0
        mv = cells.get(mp, 0)
        processor.append([clk, ip, ci, ni, mp, mv, pow(mv, P - 2, P) if mv else 0])
        executed.append([ip, ci, ni])
        if ip >= size:
            break
        op = chr(ci)
        if op == "[" and mv == 0 and enter_every_loop:
            processor[-1][6] = 1
            ip += 2
        elif op == "[":
            ip = ip + 2 if mv else ni
        elif op == "]":
            ip = ni if mv else ip + 2
        else:
            ip += 1
            if op in "<>":
                mp = (mp + (1 if op == ">" else -1)) % P
            elif op in "+-":
                cells[mp] = (mv + (1 if op == "+" else -1)) % P
            elif op == ".":
                written.append([mv])
            elif op == ",":
                cells[mp] = ord(fed.pop(0))
                read.append([cells[mp]])
        clk += 1
    listing = [[i, words[i], words[i + 1] if i + 1 < size else 0] for i in range(size)]
    instruction = sorted(listing + executed, key=lambda r: r[0])
    accesses = sorted(([r[0], r[4], r[5], 0] for r in processor if r[2]), key=lambda r: r[1])
    memory = []
    for k, row in enumerate(accesses):
        memory.append(row)
        if k + 1 < len(accesses) and accesses[k + 1][1] == row[1]:
            memory += [[c, row[1], row[2], 1] for c in range(row[0] + 1, accesses[k + 1][0])]
    return {"processor": processor, "memory": memory, "instruction": instruction, "input": read, "output": written}


WIDTHS = {"processor": 7, "memory": 4, "instruction": 3, "input": 1, "output": 1}


def _matrices_of(run):
    return {k: _wrap(run[k], WIDTHS[k]) for k in MATRICES}


def test_the_simulator_written_here_agrees_with_the_machine_when_it_is_honest():
    for code, inputs in ((CELL_PROGRAM, CELL_INPUT), ("+>[++<-]", ""), ("++[>+<-]>.", ""), (EXT_PROGRAM, EXT_INPUT)):
        _, _, matrices = _trace(code, inputs)
        run = _dishonest_run(code, inputs)
        for k in MATRICES:
            assert np.array_equal(np.array(run[k], dtype=np.uint64).reshape(-1, WIDTHS[k]), matrices[k].values[:, :WIDTHS[k]]), (code, k)


def _scenario(which):
    """(program, claim, matrices, what check_trace must name) of a false execution"""
    from stark_brainfuck_amd.vm import VirtualMachine
    if which == "every_loop_entered":
        # `+>[++<-]`: the cell under `[` is zero and the loop must be skipped; the machine enters it and runs 9 cycles instead of 4
        code = "+>[++<-]"
        run = _dishonest_run(code, enter_every_loop=True)
        honest = _dishonest_run(code)
        assert len(run["processor"]) == 9 and len(honest["processor"]) == 4 and run["processor"][-1][4] != honest["processor"][-1][4]
        assert [r[6] for r in run["processor"] if r[2] == ord("[")] == [1]
        expect = ("processor", "transition")
    elif which == "another_output":
        # the processor trace is the machine's; the output table and the claim say 3 where the program wrote 2
        code = "++[>+<-]>."
        run = _dishonest_run(code)
        assert run["output"] == [[2]]
        run["output"] = [[3]]
        expect = ("processor", "evaluation")
    else:
        # `++++`: the memory table -- one address, consecutive cycles -- may change its value from row to row as it likes as far as ITS
        # constraints go; with 0, 5, 2, 3 instead of 0, 1, 2, 3 it is no permutation of what the processor accessed
        code = "++++"
        run = _dishonest_run(code)
        assert [r[2] for r in run["memory"]] == [0, 1, 2, 3] and all(r[3] == 0 for r in run["memory"])
        run["memory"][1][2] = 5
        expect = ("processor", "permutation")
    program = VirtualMachine.compile(code)
    claim = (len(run["processor"]), len(run["memory"]), program, [], [chr(r[0]) for r in run["output"]])
    return program, claim, _matrices_of(run), expect


@pytest.mark.parametrize("which", ["every_loop_entered", "another_output", "memory_is_no_permutation"])
def test_a_coherent_false_execution_is_proven_and_refused(which, monkeypatch):
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    program, claim, matrices, expect = _scenario(which)
    violations = _flagged(claim, matrices)
    print(which, ["%s %s %d" % (v.table, v.kind, v.index) for v in violations])
    assert expect in {(v.table, v.kind) for v in violations}, violations
    if which == "memory_is_no_permutation":
        # its own AIR holds, base and extended: only the permutation argument (and the processor's terminal) knows
        assert not [v for v in violations if v.table == "memory"], violations
        assert ("processor", "permutation", 1) in {(v.table, v.kind, v.index) for v in violations}
    if which == "another_output":
        # the processor's running evaluation matches neither the claim nor the output table; every table's own AIR holds
        assert {(v.table, v.kind, v.index) for v in violations} == {("processor", "evaluation", 1), ("output", "evaluation", 1)}
    stark, proof, _ = _prove(monkeypatch, ("soundness-" + which).encode(), claim, program, matrices)          # no DEBUG: the prover goes through
    assert "quotient_buffers" not in stark._last
    _refused_alike(claim, proof)
    assert isinstance(stark, BrainfuckStark)
