"""The operands of the pointwise-kernel tests and their integer reference, without a GPU: the evaluation domain of 512 points on the
coset 7 <omega>, one table at one height with the arguments the prover would pass (Shape), the 19 operand sets (Operands: a palette
value of tests/field_states.py in every cell and scalar, palette values cycling, random residues, challenges of zero and of p - 1),
stark_brainfuck_amd/air.py evaluated on Python integers over all rows at once (constraint_values, quotients), the operands of the
difference quotient, and the exact comparison of device words with integers (assert_codeword).
tests/test_gpu_pointwise_edges.py (csrc/air.hip) and tests/compose_cases.py (csrc/compose.hip) share them."""
import random

import numpy as np

import field_states as fs
from stark_brainfuck_amd import air
from stark_brainfuck_amd.air import xscale

P = fs.P
LOG_N = 9
N = 1 << LOG_N                        # two workgroups of 256; a row's neighbour at unit distance wraps past the end
OFFSET = 7                            # the field's generator
HEIGHT = 64
PALETTE = fs.PALETTE


def primitive_root(order):
    """algebra.py:122-136: the fixed 2^32-th root of unity squared down to `order` (a power of two; 1 for order <= 1)"""
    r, o = 1753635133440165772, 1 << 32
    while o > max(order, 1):
        r, o = r * r % P, o // 2
    return r if order > 1 else 1


OMEGA = primitive_root(N)
POINTS = np.array([OFFSET * pow(OMEGA, i, P) % P for i in range(N)], dtype=object)


def inverse(v):
    return pow(int(v) % P, P - 2, P)


def inverses(values):
    return np.array([inverse(v) for v in values], dtype=object)


def full(v):
    return v if isinstance(v, np.ndarray) else np.array([int(v)] * N, dtype=object)


def to_words(values):
    return np.array([int(v) for v in np.asarray(values, dtype=object).reshape(-1)], dtype=np.uint64)


# ------------------------------------------------------------------------------------------------ shapes and operand sets
class Shape:
    """one table at one height, with the arguments the prover would pass (table.py: unit_distance, derive_omicron)"""

    def __init__(self, table, height):
        self.table, self.height = table, height
        self.air = air.TABLE_AIRS[table]
        self.bw, self.xw = self.air.base_width, self.air.full_width - self.air.base_width
        assert (self.bw, self.xw) == fs.TABLE_WIDTHS[table]
        self.kinds = [(kind, len(constraints)) for kind, constraints in self.air.all()]
        self.nq = sum(count for _, count in self.kinds)
        self.nterm = self.bw + self.xw + self.nq
        self.unit_distance = 0 if height == 0 else N // height
        self.omicron_inv = inverse(primitive_root(height))
        self.log_height = max(height.bit_length() - 1, 0)
        x = POINTS
        self.zerofier = {"boundary": inverses(x - 1), "terminal": inverses(x - self.omicron_inv),
                         "transition": full(0) if height == 0 else (x - self.omicron_inv) * inverses([pow(int(v), height, P) - 1 for v in x]) % P}

    def __repr__(self):
        return "%s-h%d" % (self.air.name, self.height)


SHAPES = [Shape(0, HEIGHT), Shape(1, HEIGHT), Shape(2, HEIGHT), Shape(3, HEIGHT), Shape(3, 0), Shape(4, HEIGHT), Shape(4, 0)]
SETS = ["palette%d" % k for k in range(len(PALETTE))] + ["cycling", "random", "challenges-zero", "challenges-p-1"]


class Operands:
    """codewords and scalars of one operand set for one table.  Every drawing goes through self.value(): a palette value, the next
    value of a cycle, or a random residue."""

    def __init__(self, shape, name):
        self.shape, self.name = shape, name
        rng = random.Random("%s/%r" % (name, shape))
        counter = iter(range(1 << 30))
        if name.startswith("palette"):
            one = PALETTE[int(name[7:])]
            scalar = cell = lambda: one
            column = lambda: full(one)
        elif name == "random":
            scalar = lambda: rng.randrange(P)
            column = lambda: np.array([rng.randrange(P) for _ in range(N)], dtype=object)
        else:                     # palette values cycling, every column and every scalar from its own phase
            scalar = lambda: PALETTE[(5 * next(counter) + 3) % len(PALETTE)]

            def column():
                phase = next(counter)
                return np.array([PALETTE[(i + 4 * phase) % len(PALETTE)] for i in range(N)], dtype=object)
        triple = lambda: (scalar(), scalar(), scalar())
        self.base = [column() for _ in range(shape.bw)]
        self.ext = [(column(), column(), column()) for _ in range(shape.xw)]
        self.challenges = [triple() for _ in range(11)]
        if name == "challenges-zero":
            self.challenges = [(0, 0, 0)] * 11
        elif name == "challenges-p-1":
            self.challenges = [(P - 1, P - 1, P - 1)] * 11
        self.terminals = [triple() for _ in range(5)]
        self.params = triple()
        self.weights = [(triple(), triple()) for _ in range(shape.nterm)]
        self.w0 = triple()
        self.randomizer = (column(), column(), column())
        self.seeded = (column(), column(), column())


def constraint_values(shape, ops, params):
    """air.evaluate over the table's three constraint lists on all rows at once -> per kind a list of triples of (N,) arrays"""
    cur = [(c, 0, 0) for c in ops.base] + list(ops.ext)
    shift = lambda a: np.roll(a, -shape.unit_distance) if isinstance(a, np.ndarray) else a
    nxt = [tuple(shift(l) for l in v) for v in cur]
    out = []
    for kind, constraints in shape.air.all():
        memo = {}
        out.append((kind, [air.evaluate(e, cur, nxt, ops.challenges, ops.terminals, [params], memo) for e in constraints]))
    return out


def quotients(shape, ops, params):
    """every quotient codeword of the table, boundary / transition / terminal order: constraint value times zerofier inverse"""
    return [tuple(full(l) for l in xscale(v, shape.zerofier[kind])) for kind, values in constraint_values(shape, ops, params) for v in values]


def assert_codeword(got, want, what):
    """(k, N) device words against k arrays of integers, exactly; every word canonical"""
    want = np.stack([to_words(full(l)) for l in want])
    assert got.shape == want.shape, what
    assert (got < np.uint64(P)).all(), "%s: words >= p" % what
    if not (got == want).all():
        plane, row = [int(v[0]) for v in np.nonzero(got != want)]
        raise AssertionError("%s differs in %d words, first in plane %d at row %d: %x, expected %x" % (
            what, int((got != want).sum()), plane, row, int(got[plane, row]), int(want[plane, row])))


# ------------------------------------------------------------------------------------------------ difference quotients
def difference_operands():
    """lhs and rhs run through every pair of palette values (row i: values i mod 15 and i div 15, rotated per limb); the
    accumulator cycles through the palette as well"""
    k = len(PALETTE)
    lhs = tuple(np.array([PALETTE[(i + l) % k] for i in range(N)], dtype=object) for l in range(3))
    rhs = tuple(np.array([PALETTE[(i // k + 2 * l) % k] for i in range(N)], dtype=object) for l in range(3))
    acc = tuple(np.array([PALETTE[(7 * i + l) % k] for i in range(N)], dtype=object) for l in range(3))
    return lhs, rhs, acc
