"""The composition kernels of prove_deep (csrc/compose.hip: bfsc_air_compose, bfsc_difference_compose) through the C ABI on codewords,
scalars and weights of the test's own choosing, against the integer model of tests/compose_cases.py (stark_brainfuck_amd/air.py on
Python integers): palette residues (tests/field_states.py) in every cell, scalar and weight, challenges of zero and of p - 1, random
residues, heights 0, 1, 64 and N, log_step 0, 1, 2 and log_n, both values of `accumulate`, h_params given and NULL, launches planted
so that the sink's unreduced sum of the boundary kind goes through every required carry state, scalars handed over unreduced, a
domain of 2^16 points, and the calls of compose_into summed into one buffer.  Every comparison is exact, every word must be < p, and
d_acc lies in a painted arena (tests/painted.py): a write beyond its 3 * (N >> log_step) words fails the test."""
import ctypes
import random

import numpy as np
import pytest

import compose_cases as cc
import field_states as fs
from painted import Arena
from pointwise_cases import (HEIGHT, LOG_N, N, OFFSET, OMEGA, PALETTE, SETS, Operands, Shape, assert_codeword, difference_operands, inverse, primitive_root,
                             to_words)
from stark_brainfuck_amd.air import xadd, xmul

pytestmark = pytest.mark.gpu

P = fs.P
u64 = ctypes.c_uint64
LOG_STEPS = (0, 1, 2, LOG_N)          # 512, 256, 128 points and one: two workgroups, one, half of one, one thread


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from stark_brainfuck_amd import _lib
    return _lib.load()            # raises BackendUnavailable if the HIP library is missing: no fallback


def ok(rc):
    from stark_brainfuck_amd import _lib
    _lib.check(rc)


def stream():
    from stark_brainfuck_amd.device import current_stream
    return current_stream()


def upload(values):
    from stark_brainfuck_amd.device import DeviceBuffer
    return DeviceBuffer.from_numpy(values if isinstance(values, np.ndarray) and values.dtype == np.uint64 else to_words(values))


def flat(triples):
    return (u64 * (3 * len(triples)))(*[int(v) for t in triples for v in t])


def accumulator(count, start):
    """a painted arena of three planes of `count` words; start: None (paint: the call must not read it) or three arrays to add onto"""
    arena = Arena(batch=3, stride=count, n=count)
    if start is not None:
        arena.fill(0, to_words(np.concatenate([np.asarray(l, dtype=object) for l in start])))
    return arena


def result(arena, want, what):
    """nothing outside the three planes changed; the planes equal `want` exactly"""
    assert_codeword(arena.rows(arena.contained()), want, what)


class Launch:
    """device codewords and host scalars of one operand set for one table: compose() is one bfsc_air_compose call"""

    def __init__(self, shape, ops, weights=None):
        self.shape, self.ops = shape, ops
        self.weights = cc.compose_weights(shape, ops) if weights is None else weights
        self.d_base, self.d_ext = upload(ops.base), upload(ops.ext)

    def compose(self, lib, arena, log_step, accumulate, params, lift=lambda v: v):
        s, ops = self.shape, self.ops
        lifted = lambda triples: flat([[lift(v) for v in t] for t in triples])
        ok(lib.bfsc_air_compose(s.table, self.d_base.ptr, self.d_ext.ptr, LOG_N, s.unit_distance, s.height, lift(s.omicron_inv), lift(OFFSET), OMEGA,
                                lifted(ops.challenges), lifted(ops.terminals), None if params is None else lifted([params]), lifted(self.weights),
                                log_step, accumulate, arena.ptr, stream()))

    def reference(self, log_step, start, params):
        return cc.compose_reference(self.shape, self.ops, self.weights, params, log_step, start)


def every(step, planes):
    return [l[::step] for l in planes]


def check_launch(lib, launch, what, log_steps=LOG_STEPS):
    """every log_step, into paint and onto the set's seeded residues, with the parameter and (where the table reads one) without"""
    shape, ops = launch.shape, launch.ops
    for params in ((ops.params, None) if shape.air.num_params else (ops.params,)):
        whole = launch.reference(0, None, params)
        for log_step in log_steps:
            step, count = 1 << log_step, N >> log_step
            for accumulate in (0, 1):
                start = every(step, ops.seeded) if accumulate else None
                want = every(step, whole) if start is None else [(a + b) % P for a, b in zip(every(step, whole), start)]
                arena = accumulator(count, start)
                launch.compose(lib, arena, log_step, accumulate, params)
                result(arena, want, "%s%s, log_step %d, accumulate %d" % (what, "" if params is not None else " (params NULL)", log_step, accumulate))


# ------------------------------------------------------------------------------------------------ chosen codewords
@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("shape", cc.COMPOSE_SHAPES, ids=repr)
def test_composition_on_chosen_codewords(lib, shape, name):
    check_launch(lib, Launch(shape, Operands(shape, name)), "%r %s" % (shape, name))


# ------------------------------------------------------------------------------------------------ planted launches
@pytest.mark.parametrize("table", cc.PLANTED_TABLES, ids=lambda t: "table%d" % t)
def test_planted_launches_reach_every_required_sink_state(lib, table):
    launches = cc.planted_launches(table)
    acc, inner = set(), set()
    for ops in launches:
        a, r = cc.boundary_states(ops)
        acc |= a
        inner |= r
    want_acc, want_inner = cc.BOUNDARY_FLOOR[table]
    assert want_acc <= acc, sorted(want_acc - acc)
    assert want_inner <= inner, sorted(want_inner - inner)
    for ops in launches:
        weights = cc.compose_weights(ops.shape, ops)
        assert all(any(w) for w in weights[ops.shape.kinds[0][1]:]), "transition and terminal weights must not be zero"
        check_launch(lib, Launch(ops.shape, ops, weights), "%r %s" % (ops.shape, ops.name), log_steps=(0,))


# ------------------------------------------------------------------------------------------------ scalars handed over unreduced
def test_scalars_at_and_above_p_are_reduced(lib):
    """word + p in place of every scalar word that leaves room for it in 64 bits (word < 2^32 - 1); every fourth scalar word (so that the limb rotates) is made
    that small first, the edges 0 and 2^32 - 2 among them"""
    room = (1 << 32) - 1
    lift = lambda v: int(v) + P if int(v) < room else int(v)
    for shape in (Shape(0, 1), Shape(1, HEIGHT), Shape(2, 1), Shape(3, HEIGHT), Shape(4, 1)):
        ops = Operands(shape, "random")
        rng = random.Random("small words/%r" % shape)
        small = iter(range(1 << 30))
        edges = (0, room - 1, 1)

        def some_small(triples):
            out = []
            for t in triples:
                words = []
                for v in t:
                    k = next(small)
                    words.append((edges[k // 4 % 3] if k < 36 else rng.randrange(room)) if k % 4 == 0 else v)
                out.append(tuple(words))
            return out
        ops.challenges, ops.terminals, (ops.params,) = some_small(ops.challenges), some_small(ops.terminals), some_small([ops.params])
        launch = Launch(shape, ops, some_small(cc.compose_weights(shape, ops)))
        scalars = [v for t in ops.challenges + ops.terminals + [ops.params] + launch.weights for v in t]
        assert sum(1 for v in scalars if v < room) >= len(scalars) // 4 and lift(OFFSET) == OFFSET + P
        assert all(lift(v) < 1 << 64 and lift(v) % P == v for v in scalars + [shape.omicron_inv])
        if shape.height == 1:
            assert lift(shape.omicron_inv) == 1 + P
        for log_step, accumulate in ((0, 0), (2, 1)):
            step = 1 << log_step
            start = every(step, ops.seeded) if accumulate else None
            want = launch.reference(log_step, start, ops.params)
            outputs = []
            for how in (lambda v: v, lift):
                arena = accumulator(N >> log_step, start)
                launch.compose(lib, arena, log_step, accumulate, ops.params, lift=how)
                outputs.append(arena.rows(arena.contained()))
            what = "%r, log_step %d, accumulate %d" % (shape, log_step, accumulate)
            assert_codeword(outputs[0], want, what + ", canonical scalars")
            assert np.array_equal(outputs[0], outputs[1]), what + ": scalars + p change the output"


# ------------------------------------------------------------------------------------------------ difference quotients
@pytest.mark.parametrize("k", range(len(PALETTE)))
def test_difference_compose_on_palette_operands(lib, k):
    """every pair of palette values in lhs and rhs, the weight three palette values rotated by k, onto paint and onto the palette"""
    lhs, rhs, acc = difference_operands()
    assert {(int(a), int(b)) for a, b in zip(lhs[0], rhs[0])} == set(fs.palette_pairs())
    weight = tuple(PALETTE[(k + l) % len(PALETTE)] for l in range(3))
    d_lhs, d_rhs = upload(lhs), upload(rhs)
    for log_step in (0, 1, LOG_N):
        step = 1 << log_step
        for accumulate in (0, 1):
            start = every(step, acc) if accumulate else None
            arena = accumulator(N >> log_step, start)
            ok(lib.bfsc_difference_compose(d_lhs.ptr, d_rhs.ptr, LOG_N, OFFSET, OMEGA, flat([weight]), log_step, accumulate, arena.ptr, stream()))
            result(arena, cc.difference_reference(lhs, rhs, weight, log_step, start), "difference compose, palette %d, log_step %d, accumulate %d" % (k, log_step, accumulate))
    # the weight and the offset unreduced
    lift = lambda v: v + P if v < (1 << 32) - 1 else v
    arena = accumulator(N, None)
    ok(lib.bfsc_difference_compose(d_lhs.ptr, d_rhs.ptr, LOG_N, lift(OFFSET), OMEGA, flat([[lift(v) for v in weight]]), 0, 0, arena.ptr, stream()))
    result(arena, cc.difference_reference(lhs, rhs, weight, 0, None), "difference compose, palette %d, weight and offset + p" % k)


# ------------------------------------------------------------------------------------------------ 2^16 points
def test_composition_at_2_16(lib):
    """the processor table at height 2^12 on 2^16 points, then a difference quotient added onto it: all 4096 points of log_step 4;
    at log_step 0 one point in every 16 -- the low exponent bits running through all their values, so that the exponent of offset *
    omega^i goes through both halves of the two-level power table wherever it is split -- and both ends of the first, a middle and the
    last workgroup.  The model sees only those rows."""
    log_n, height, table = 16, 1 << 12, 0
    n = 1 << log_n
    omega = primitive_root(n)
    shape = Shape(table, HEIGHT)          # widths and quotient count only
    rng = np.random.default_rng(20260116)
    base = rng.integers(0, P, size=(shape.bw, n), dtype=np.uint64)
    ext = rng.integers(0, P, size=(shape.xw, 3, n), dtype=np.uint64)
    lhs, rhs = ext[1], ext[3]
    draw = random.Random("2^16")
    triple = lambda: tuple(draw.randrange(P) for _ in range(3))
    challenges, terminals, weights, beta = [triple() for _ in range(11)], [triple() for _ in range(5)], [triple() for _ in range(shape.nq)], triple()
    stepped = [16 * k for k in range(n >> 4)]
    spread = sorted(set([16 * k + 5 * k % 16 for k in range(n >> 4)] + [0, 255, n // 2, n // 2 + 255, n - 256, n - 1]))
    assert {i % 16 for i in spread} == set(range(16)) and {i >> 12 for i in spread} == set(range(16))
    rows = sorted(set(stepped + spread))
    where = {i: at for at, i in enumerate(rows)}
    total = cc.compose_reference_rows(table, log_n, OFFSET, height, base, ext, challenges, terminals, None, weights, rows)
    x = [OFFSET * pow(omega, i, P) % P for i in rows]
    quotient = tuple(np.array([(int(a[i]) - int(b[i])) * inverse(v - 1) % P for i, v in zip(rows, x)], dtype=object) for a, b in zip(lhs, rhs))
    total = xadd(tuple(total), xmul(beta, quotient))
    d_base, d_ext = upload(base.reshape(-1)), upload(ext.reshape(-1))
    for log_step, points in ((4, stepped), (0, spread)):
        count = n >> log_step
        arena = Arena(batch=3, stride=count, n=count)
        ok(lib.bfsc_air_compose(table, d_base.ptr, d_ext.ptr, log_n, n // height, height, inverse(primitive_root(height)), OFFSET, omega,
                                flat(challenges), flat(terminals), None, flat(weights), log_step, 0, arena.ptr, stream()))
        ok(lib.bfsc_difference_compose(d_ext.ptr + 8 * 3 * n, d_ext.ptr + 8 * 9 * n, log_n, OFFSET, omega, flat([beta]), log_step, 1, arena.ptr, stream()))
        got = arena.rows(arena.contained())
        assert (got < np.uint64(P)).all(), "log_step %d: words >= p" % log_step
        at = [where[i] for i in points]
        assert_codeword(got[:, [i >> log_step for i in points]], [l[at] for l in total], "2^16 points, log_step %d" % log_step)


# ------------------------------------------------------------------------------------------------ one buffer, call after call
@pytest.mark.parametrize("name", ["random", "cycling"])
def test_tables_composed_one_after_the_other_are_the_sum(lib, name):
    """the calls of BrainfuckStark.compose_into with none skipped: the five tables at heights 64, 64, 64, 0 and 1, then two difference
    quotients; the first call writes into paint, the others add.  The table of height 0 contributes its boundary and terminal
    quotients and no transition quotient."""
    log_step = 2
    launches = [Launch(shape, Operands(shape, name)) for shape in (Shape(0, HEIGHT), Shape(1, HEIGHT), Shape(2, HEIGHT), Shape(3, 0), Shape(4, 1))]
    lhs, rhs, _ = difference_operands()
    differences = [(lhs, rhs, launches[0].ops.w0), (rhs, launches[2].ops.seeded, launches[1].ops.w0)]
    arena = accumulator(N >> log_step, None)
    want, accumulate = None, 0
    for launch in launches:
        launch.compose(lib, arena, log_step, accumulate, launch.ops.params)
        want = launch.reference(log_step, want, launch.ops.params)
        accumulate = 1
    for lhs_, rhs_, weight in differences:
        d_lhs, d_rhs = upload(lhs_), upload(rhs_)
        ok(lib.bfsc_difference_compose(d_lhs.ptr, d_rhs.ptr, LOG_N, OFFSET, OMEGA, flat([weight]), log_step, 1, arena.ptr, stream()))
        want = cc.difference_reference(lhs_, rhs_, weight, log_step, want)
    result(arena, want, "seven calls into one buffer, set %s" % name)
    # the height-0 branch by itself: the transition weights do not matter
    height_0 = launches[3]
    alone = accumulator(N >> log_step, None)
    height_0.compose(lib, alone, log_step, 0, height_0.ops.params)
    zeroed = Launch(height_0.shape, height_0.ops, [w if keep else (0, 0, 0) for w, keep in zip(height_0.weights, transition_mask(height_0.shape))])
    result(alone, zeroed.reference(log_step, None, height_0.ops.params), "height 0 alone, set %s" % name)


def transition_mask(shape):
    """per quotient: False for the transition quotients"""
    return [kind != "transition" for kind, count in shape.kinds for _ in range(count)]
