"""The composition kernels of a proof by out-of-domain openings (csrc/compose.hip: bfsc_air_compose, bfsc_difference_compose) in
Python integers, and the cases the tests run them on.  No GPU and none of the product's C++: the statement is
stark_brainfuck_amd/air.py through tests/pointwise_cases.py, the carry model tests/field_states.py.

  compose_reference      H on every 2^log_step-th point of the 512-point domain: start + sum over the kinds of
                         zerofier_inverse[kind] * sum_q beta_q * value_q
  compose_reference_rows the same on chosen rows of a domain of any size (the 2^16 test hands over only the rows it compares)
  difference_reference   start + beta * (lhs - rhs) / (x - 1)
  kind_streams           what ComposeSink multiplies: per kind and per limb of the accumulator the (value word, weight word) pairs
                         in quotient order -- (v, w[l]) for a base-valued quotient, the three products of fs.EXT_WORDS over
                         fs.weight_matrix(w) for an extension-valued one.  A quotient is extension-valued when its expression in
                         air.py mentions an extension column, a challenge, a terminal or a parameter (q_ext); the host test holds
                         that against the *_Q_EXT arrays of csrc/air_generated.hpp (generated_q_ext), which is what lays the
                         weights out on the device.
  compose_states         fs.lazy_sum over those streams, row by row: the values and the (accumulator, inner) carry states per kind

Every value that reaches the sink is canonical: the boundary values of the processor and memory tables are bare cells, and every
other value leaves the generated code through gl_add / gl_sub / gl_mul or an xfe_ operation made of them (csrc/gl.hpp), all of which
return residues below p.  So the streams carry air.py's residues as they are.

Shapes: the seven of pointwise_cases plus heights 1 (omicron = 1: the boundary and terminal zerofiers coincide, the transition
factor is 1, the row after a row is the row itself) and N (unit distance 1).

Planted launches (processor and memory).  The boundary values of these two tables are bare cells, so a sum of k products can be
aimed at the boundary kind's accumulator exactly as fs.designed_launch aims the column sums: the first operands go into the boundary
cells (limb 0 of an extension cell, its other limbs zero) of the rows fs.WITNESS_ROWS, all other boundary cells of those rows zero, the
second operands into word l of the first k boundary weights.  The designed launch is planted_launch(table, 0) with the witnesses of
fs.ACC_WITNESSES / fs.ACC_INNER_WITNESSES written in; launches of further seeds are kept while they add a state (planted_search).
Every other cell, weight, challenge and terminal of a launch is a palette value, the transition and terminal weights included: the
sink closes and reopens its sum at both kind boundaries.

Floors.  BOUNDARY_FLOOR is what the planted launches must reach in the boundary kind: all of fs.ACC_REQUIRED and
fs.ACC_INNER_REQUIRED for the processor table (11 products per limb); for the memory table (3 products per limb) the whole inner floor
and the accumulator floor without MEMORY_UNREACHED -- (0,1,1,1,0), (0,1,1,1,1) and (1,1,0,1,0), which no sum of three products of
palette values reaches (all 1.9 million multisets of three of the 225 pairs were tried); the shortest known witness of (1,1,0,1,0)
has five products.  REACHED pins, for every other (table, kind), what the 19 operand sets over the table's shapes together with the
planted launches reach; there are no aimed sums for them, and tests/test_compose_cases_host.py keeps the literal from shrinking."""
import functools
import os
import random
import re

import numpy as np

import field_states as fs
from pointwise_cases import HEIGHT, N, PALETTE, POINTS, SETS, SHAPES, Operands, Shape, constraint_values, full, inverse, inverses, primitive_root
from stark_brainfuck_amd import air
from stark_brainfuck_amd.air import xadd, xmul, xscale

P = fs.P
COMPOSE_SHAPES = SHAPES + [Shape(0, 1), Shape(2, 1), Shape(4, 1), Shape(0, N), Shape(1, N)]
KINDS = ("boundary", "transition", "terminal")
NO_PARAMS = (1, 0, 0)                 # what a NULL h_params stands for


# ------------------------------------------------------------------------------------------------ which quotients are extension-valued
def mentions_extension(e, base_width, memo=None):
    """whether expression e reads an extension column, a challenge, a terminal or a parameter"""
    memo = {} if memo is None else memo
    if id(e) not in memo:
        if e.op == "v":
            r = e.val[0] >= base_width
        elif e.op == "k":
            r = False
        elif e.op in ("c", "t", "p"):
            r = True
        else:
            r = mentions_extension(e.a, base_width, memo) or (e.b is not None and mentions_extension(e.b, base_width, memo))
        memo[id(e)] = r
    return memo[id(e)]


@functools.lru_cache(maxsize=None)
def q_ext(table):
    """per quotient of the table, boundary / transition / terminal order: is its value an extension element?"""
    a = air.TABLE_AIRS[table]
    return tuple(mentions_extension(e, a.base_width) for _, constraints in a.all() for e in constraints)


def generated_header():
    return open(os.path.join(os.path.dirname(os.path.abspath(air.__file__)), "csrc", "air_generated.hpp")).read()


def generated_q_ext():
    """{table name: tuple of bool} as csrc/air_generated.hpp states it (NAME_Q_EXT[])"""
    found = re.findall(r"constexpr bool (\w+)_Q_EXT\[\] = \{([^}]*)\};", generated_header())
    return {name.lower(): tuple({"true": True, "false": False}[v.strip()] for v in body.split(",")) for name, body in found}


def generated_num_quotients():
    """{table name: boundary + transition + terminal constraints} of the header: what bfs_air_num_quotients returns"""
    found = re.findall(r"(\w+)_NUM_BOUNDARY = (\d+), \w+_NUM_TRANSITION = (\d+), \w+_NUM_TERMINAL = (\d+);", generated_header())
    return {name.lower(): int(b) + int(t) + int(z) for name, b, t, z in found}


# ------------------------------------------------------------------------------------------------ the reference
def compose_weights(shape, ops):
    """one triple per quotient from the operand set's own scalars: the first weight of the set's quotient terms"""
    return [ops.weights[shape.bw + shape.xw + q][0] for q in range(shape.nq)]


def add_start(total, start, step):
    out = [full(l)[::step] for l in total]
    return out if start is None else [(a + np.asarray(b, dtype=object)) % P for a, b in zip(out, start)]


def compose_reference(shape, ops, weights, params, log_step, start):
    """three arrays of N >> log_step integers: start[k] + sum_kind zerofier_inverse[kind][i] * sum_q beta_q * value_q[i] at
    i = k << log_step; params None is a NULL h_params, start None an accumulator that is not read"""
    assert len(weights) == shape.nq
    total, at = (0, 0, 0), 0
    for kind, values in constraint_values(shape, ops, NO_PARAMS if params is None else params):
        weighted = (0, 0, 0)
        for v in values:
            weighted = xadd(weighted, xmul(weights[at], v))
            at += 1
        total = xadd(total, xscale(weighted, shape.zerofier[kind]))
    return add_start(total, start, 1 << log_step)


def compose_reference_rows(table, log_n, offset, height, base, ext, challenges, terminals, params, weights, rows):
    """H of one table at the points offset * omega^i, i in rows, of a domain of 2^log_n points; base[c] and ext[c][limb] are whole
    codewords (anything indexable by an integer array), read only at the rows and at their neighbours at unit distance"""
    n = 1 << log_n
    rows = np.asarray(rows, dtype=np.int64)
    after = (rows + (n // height if height else 0)) % n
    take = lambda column, where: np.array([int(v) for v in np.asarray(column)[where]], dtype=object)
    cur = [(take(c, rows), 0, 0) for c in base] + [tuple(take(l, rows) for l in c) for c in ext]
    nxt = [(take(c, after), 0, 0) for c in base] + [tuple(take(l, after) for l in c) for c in ext]
    omega, omicron_inv = primitive_root(n), inverse(primitive_root(height))
    x = np.array([offset * pow(omega, int(i), P) % P for i in rows], dtype=object)
    zerofier = {"boundary": inverses(x - 1), "terminal": inverses(x - omicron_inv),
                "transition": 0 if height == 0 else (x - omicron_inv) * inverses([pow(int(v), height, P) - 1 for v in x]) % P}
    total, at = (0, 0, 0), 0
    for kind, constraints in air.TABLE_AIRS[table].all():
        memo, weighted = {}, (0, 0, 0)
        for e in constraints:
            weighted = xadd(weighted, xmul(weights[at], air.evaluate(e, cur, nxt, challenges, terminals, [NO_PARAMS if params is None else params], memo)))
            at += 1
        total = xadd(total, xscale(weighted, zerofier[kind]))
    assert at == len(weights)
    return [l if isinstance(l, np.ndarray) else np.array([int(l)] * len(rows), dtype=object) for l in total]


def difference_reference(lhs, rhs, weight, log_step, start, points=POINTS):
    """start[k] + weight * (lhs - rhs)(x_i) / (x_i - 1), i = k << log_step, over the codewords' whole domain `points`"""
    quotient = xscale(tuple((a - b) % P for a, b in zip(lhs, rhs)), inverses(points - 1))
    return add_start(xmul(weight, quotient), start, 1 << log_step)


# ------------------------------------------------------------------------------------------------ what the sink multiplies
def kind_streams(shape, ops, weights, params):
    """[(kind, (stream 0, stream 1, stream 2))]: stream l holds the (value, weight word) pairs of limb l of the kind's unreduced sum
    in the order ComposeSink consumes them; a value is an array over the rows or one integer.  Takes exactly one weight per quotient."""
    supply = iter(weights)
    ext, at, out = q_ext(shape.table), 0, []
    for kind, values in constraint_values(shape, ops, NO_PARAMS if params is None else params):
        streams = ([], [], [])
        for v in values:
            w = next(supply, None)
            assert w is not None, "%r: fewer weights than quotients" % shape
            if ext[at]:
                m = fs.weight_matrix(w)
                for l in range(3):
                    streams[l].extend((v[k], m[fs.EXT_WORDS[l][k]]) for k in range(3))
            else:
                assert not np.any(v[1]) and not np.any(v[2]), "%r: quotient %d is not base-valued" % (shape, at)
                for l in range(3):
                    streams[l].append((v[0], w[l]))
            at += 1
        out.append((kind, streams))
    assert next(supply, None) is None, "%r: more weights than quotients" % shape
    return out


def reduce_streams(streams, rows=None):
    """fs.lazy_sum over the three streams of a kind on every row of `rows` (default: all) -> (three lists of values, accumulator
    states, inner states).  Equal sums are reduced once: a palette set has one distinct row."""
    rows = range(N) if rows is None else rows
    values, acc, inner, seen = [], set(), set(), {}
    for stream in streams:
        split = [(v, int(w)) if isinstance(v, np.ndarray) else (None, (int(v), int(w))) for v, w in stream]
        limb = []
        for i in rows:
            pairs = tuple(fixed if v is None else (int(v[i]), fixed) for v, fixed in split)
            hit = seen.get(pairs)
            if hit is None:
                hit = seen[pairs] = fs.lazy_sum(pairs)
            limb.append(hit[0])
            acc.add(hit[1][0])
            inner.add(hit[1][1])
        values.append(limb)
    return values, acc, inner


def compose_states(shape, ops, weights, params, rows=None):
    """{kind: (accumulator states, inner states)} of the sink's three sums"""
    return {kind: reduce_streams(streams, rows)[1:] for kind, streams in kind_streams(shape, ops, weights, params)}


# ------------------------------------------------------------------------------------------------ planted launches
PLANTED_TABLES = (0, 2)               # processor and memory: the tables whose boundary values are bare cells
PLANTED_TRIES = 40


def boundary_cells(shape, ops):
    """the arrays behind the boundary values of a table whose boundary constraints are bare cells, in quotient order: (limb 0, other
    limbs) per value -- a base column and (), or the three limbs of an extension column"""
    cells = []
    for e in shape.air.boundary():
        assert e.op == "v" and not e.val[1], "%r: a boundary constraint that is not a bare cell" % shape
        c = e.val[0]
        cells.append((ops.base[c], ()) if c < shape.bw else (ops.ext[c - shape.bw][0], ops.ext[c - shape.bw][1:]))
    return cells


def planted_launch(table, seed):
    """operands for one launch at height 64 with every cell, weight, challenge, terminal and parameter drawn from the palette"""
    shape = Shape(table, HEIGHT)
    rng = random.Random((seed << 3) | table)
    pick = lambda: rng.choice(PALETTE)
    triple = lambda: (pick(), pick(), pick())
    column = lambda: np.array([pick() for _ in range(N)], dtype=object)
    ops = Operands.__new__(Operands)
    ops.shape, ops.name = shape, "planted-%d" % seed
    ops.weights = [((0, 0, 0), (0, 0, 0))] * (shape.bw + shape.xw) + [(triple(), (0, 0, 0)) for _ in range(shape.nq)]
    ops.base = [column() for _ in range(shape.bw)]
    ops.ext = [(column(), column(), column()) for _ in range(shape.xw)]
    ops.challenges, ops.terminals, ops.params = [triple() for _ in range(11)], [triple() for _ in range(5)], triple()
    ops.seeded = (column(), column(), column())
    return ops


def designed_launch(table):
    """planted_launch(table, 0) with witness sums in the boundary kind: limb 0 carries the accumulator witness of (1, 1, 0, 1, 0)
    where the kind has the five products for it (the inner (1, 1, 0, 0) one where it has not), limb 1 the inner (1, 1, 0, 1) one;
    the rows fs.WITNESS_ROWS alternate between them"""
    ops = planted_launch(table, 0)
    shape = ops.shape
    cells = boundary_cells(shape, ops)
    wide = fs.ACC_WITNESSES[(1, 1, 0, 1, 0)]
    per_limb = [wide if len(wide) <= len(cells) else fs.ACC_INNER_WITNESSES[(1, 1, 0, 0)], fs.ACC_INNER_WITNESSES[(1, 1, 0, 1)]]
    first = shape.bw + shape.xw
    for limb, pairs in enumerate(per_limb):
        for k, (_, b) in enumerate(pairs):
            beta = list(ops.weights[first + k][0])
            beta[limb] = b
            ops.weights[first + k] = (tuple(beta), (0, 0, 0))
    for number, row in enumerate(fs.WITNESS_ROWS):
        pairs = per_limb[number % 2]
        for k, (cell, others) in enumerate(cells):
            cell[row] = pairs[k][0] if k < len(pairs) else 0
            for other in others:
                other[row] = 0
    return ops


def boundary_states(ops):
    return compose_states(ops.shape, ops, compose_weights(ops.shape, ops), ops.params)["boundary"]


MEMORY_UNREACHED = frozenset([(0, 1, 1, 1, 0), (0, 1, 1, 1, 1), (1, 1, 0, 1, 0)])      # need more than the kind's three products
BOUNDARY_FLOOR = {0: (fs.ACC_REQUIRED, fs.ACC_INNER_REQUIRED), 2: (fs.ACC_REQUIRED - MEMORY_UNREACHED, fs.ACC_INNER_REQUIRED)}


def planted_search(table, first_seed=1, tries=PLANTED_TRIES):
    """fs.planted_search's rule on the boundary kind: the launches of seeds first_seed, first_seed + 1, ... are kept while they add
    a state to what the designed launch and the kept ones reach; stops at the table's floor or after `tries` launches.
    Returns (seeds kept, accumulator states, inner states)."""
    want_acc, want_inner = BOUNDARY_FLOOR[table]
    acc, inner = (set(s) for s in boundary_states(designed_launch(table)))
    kept = []
    for seed in range(first_seed, first_seed + tries):
        if want_acc <= acc and want_inner <= inner:
            break
        a, r = boundary_states(planted_launch(table, seed))
        if (a - acc) or (r - inner):
            kept.append(seed)
            acc |= a
            inner |= r
    return tuple(kept), acc, inner


# planted_search(table) for the two tables (tests/test_compose_cases_host.py runs the memory table's again)
PLANTED_SEEDS = {0: (3, 30), 2: (2, 3, 6, 10, 19, 25)}


def planted_launches(table):
    """the launches the GPU test plants for `table`: the designed one, then the seeds the search kept"""
    return [designed_launch(table)] + [planted_launch(table, seed) for seed in PLANTED_SEEDS[table]]


# ------------------------------------------------------------------------------------------------ what the other sums reach
def reached_states():
    """{(table, kind): (accumulator states, inner states)} over every shape of COMPOSE_SHAPES on the 19 operand sets, with and
    without the parameter where the table has one, and over the planted launches"""
    out = {(table, kind): (set(), set()) for table in range(5) for kind in KINDS}

    def note(table, states):
        for kind, (acc, inner) in states.items():
            out[table, kind][0].update(acc)
            out[table, kind][1].update(inner)
    for shape in COMPOSE_SHAPES:
        for name in SETS:
            ops = Operands(shape, name)
            for params in ((ops.params, None) if shape.air.num_params else (ops.params,)):
                note(shape.table, compose_states(shape, ops, compose_weights(shape, ops), params))
    for table in PLANTED_TABLES:
        for ops in planted_launches(table):
            note(table, compose_states(ops.shape, ops, compose_weights(ops.shape, ops), ops.params))
    return out


REACHED = {
    (0, 'transition'): (frozenset([(0, 0, 0, 0, 0), (0, 0, 0, 1, 0)]),
        frozenset([(0, 0, 0, 0), (0, 0, 1, 0)])),
    (0, 'terminal'): (frozenset([(0, 0, 0, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 1, 1), (0, 0, 1, 1, 0), (1, 0, 0, 1, 0)]),
        frozenset([(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0)])),
    (1, 'boundary'): (frozenset([(0, 0, 0, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 1, 1), (0, 0, 1, 1, 0), (0, 1, 0, 0, 0), (1, 0, 0, 1, 0)]),
        frozenset([(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (1, 0, 0, 1), (1, 0, 1, 0)])),
    (1, 'transition'): (frozenset([(0, 0, 0, 0, 0), (0, 0, 0, 1, 0)]),
        frozenset([(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0)])),
    (1, 'terminal'): (frozenset([(0, 0, 0, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 1, 1), (1, 0, 0, 1, 0)]),
        frozenset([(0, 0, 0, 0), (0, 0, 1, 0)])),
    (2, 'transition'): (frozenset([(0, 0, 0, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 1, 1), (0, 0, 1, 1, 0), (0, 0, 1, 1, 1), (0, 1, 0, 0, 0), (0, 1, 0, 1, 0), (1, 0, 0, 1, 0)]),
        frozenset([(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (1, 0, 1, 0)])),
    (2, 'terminal'): (frozenset([(0, 0, 0, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 1, 1), (0, 0, 1, 1, 0), (0, 1, 0, 0, 0), (0, 1, 0, 1, 0), (1, 0, 0, 1, 0)]),
        frozenset([(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (1, 0, 0, 1), (1, 0, 1, 0), (1, 1, 1, 0)])),
    (3, 'boundary'): (frozenset([(0, 0, 0, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 1, 1)]),
        frozenset([(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (1, 0, 0, 1), (1, 0, 1, 0)])),
    (3, 'transition'): (frozenset([(0, 0, 0, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 1, 1), (0, 0, 1, 1, 0), (0, 1, 0, 1, 0), (1, 0, 0, 1, 0)]),
        frozenset([(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (1, 0, 0, 1), (1, 0, 1, 0)])),
    (3, 'terminal'): (frozenset([(0, 0, 0, 0, 0), (0, 0, 0, 1, 0), (0, 0, 1, 1, 0), (0, 0, 1, 1, 1), (1, 0, 0, 1, 0)]),
        frozenset([(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0)])),
    (4, 'boundary'): (frozenset([(0, 0, 0, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 1, 1)]),
        frozenset([(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (1, 0, 0, 1), (1, 0, 1, 0)])),
    (4, 'transition'): (frozenset([(0, 0, 0, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 1, 1), (0, 0, 1, 1, 0), (0, 1, 0, 1, 0), (1, 0, 0, 1, 0)]),
        frozenset([(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (1, 0, 0, 1), (1, 0, 1, 0)])),
    (4, 'terminal'): (frozenset([(0, 0, 0, 0, 0), (0, 0, 0, 1, 0), (0, 0, 1, 1, 0), (0, 0, 1, 1, 1), (1, 0, 0, 1, 0)]),
        frozenset([(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0)])),
}
