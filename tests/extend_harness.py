"""What the host and the GPU tests of the extension stage share: the package's table classes built from a case of extend_cases.py, the
model's answer for a case (computed once), and the tables' extensions in scan form."""
import functools

import numpy as np

import extend_cases
import extend_model
from scan_model import P

ALL_CASES = {c["name"]: c for c in extend_cases.all_cases()}


@functools.lru_cache(maxsize=None)
def expected(name):
    """extend_model on a case, computed once: (columns, terminals)"""
    return extend_model.extend(ALL_CASES[name])


def planes(column):
    """a model column (one triple per row) as the (3, rows) array of limb planes the package keeps"""
    return np.array(column, dtype=np.uint64).reshape(len(column), 3).T


def make_table(case):
    """the package's table class for a case, `matrix` set as _lde_case of test_gpu_stark.py sets it"""
    from stark_brainfuck_amd.algebra import BaseField
    from stark_brainfuck_amd.instruction_table import InstructionTable
    from stark_brainfuck_amd.io_table import InputTable, OutputTable
    from stark_brainfuck_amd.memory_table import MemoryTable
    from stark_brainfuck_amd.processor_table import ProcessorTable
    field, order = BaseField.main(), 1 << 32
    generator, h = field.primitive_nth_root(order), case["height"]
    if case["table"] in ("input", "output"):
        t = (InputTable if case["table"] == "input" else OutputTable)(field, h, generator, order)
        t.length = case["length"]
    else:
        cls = {"processor": ProcessorTable, "instruction": InstructionTable, "memory": MemoryTable}[case["table"]]
        t = cls(field, h, 1, generator, order)
    t.matrix = [list(row) for row in case["matrix"]]
    assert t.height == h == len(t.matrix)
    return t


def table_terminals(t, table):
    if table == "processor":
        return [t.instruction_permutation_terminal, t.memory_permutation_terminal, t.input_evaluation_terminal, t.output_evaluation_terminal]
    if table == "instruction":
        return [t.permutation_terminal, t.evaluation_terminal]
    return [t.permutation_terminal] if table == "memory" else [t.evaluation_terminal]


def scan_statement(case):
    """a table's extension as scans of scan_model (kind, columns, mask, constants, initial, before, shift1) -- the form the package uses,
    written here to derive NEIGHBOURING rules from it (test_extend_host.py, which also holds it equal to extend_model) and to name the
    masks bfs_trace_pad has to write (test_gpu_extend.py)"""
    m, ch, (i0, i1) = case["matrix"], case["challenges"], case["initials"]
    a, b, c, d, e, f, alpha, beta, gamma, delta, eta = ch
    col = lambda k: [row[k] for row in m]
    one = (1, 0, 0)
    if case["table"] == "processor":
        active = [row[2] != 0 for row in m]
        return [(0, [col(1), col(2), col(3)], active, [alpha, a, b, c], i0, True, 0), (0, [col(0), col(4), col(5)], active, [beta, d, e, f], i1, True, 0),
                (1, [col(5)], [row[2] == ord(",") for row in m], [gamma, one], (0, 0, 0), True, 1),
                (1, [col(5)], [row[2] == ord(".") for row in m], [delta, one], (0, 0, 0), True, 0)]
    if case["table"] == "instruction":
        same = [i > 0 and m[i][0] == m[i - 1][0] for i in range(len(m))]
        first = [not s and not (i == 0 and m[0][0] == P - 1) for i, s in enumerate(same)]
        return [(0, [col(0), col(1), col(2)], [s and row[1] != 0 for s, row in zip(same, m)], [alpha, a, b, c], i0, False, 0),
                (1, [col(0), col(1), col(2)], first, [eta, a, b, c], (0, 0, 0), False, 0)]
    if case["table"] == "memory":
        return [(0, [col(0), col(1), col(2)], [row[3] == 0 for row in m], [beta, d, e, f], i1, True, 0)]
    return [(1, [col(0)], None, [gamma if case["table"] == "input" else delta, one], (0, 0, 0), False, 0)]
