"""tests/compose_cases.py without a GPU: the integer model of the composition kernels agrees with itself by three routes, its reading
of which quotients are extension-valued is the generated header's, it takes one weight per quotient, and the planted launches and
the operand sets reach the sink states the module pins."""
import numpy as np
import pytest

import compose_cases as cc
import field_states as fs
from pointwise_cases import LOG_N, N, OFFSET, SHAPES, Operands, quotients, to_words
from stark_brainfuck_amd import air
from stark_brainfuck_amd.air import xadd, xmul, xscale

P = fs.P
ROUTE_SETS = ("cycling", "random", "palette8", "palette14")


def same(got, want, what):
    got, want = [to_words(l) for l in got], [to_words(l) for l in want]
    assert all(g.shape == w.shape and (g == w).all() for g, w in zip(got, want)), what


@pytest.mark.parametrize("shape", cc.COMPOSE_SHAPES, ids=repr)
def test_the_model_agrees_with_itself_by_three_routes(shape):
    """the kernel's route (unreduced sums per kind through fs.lazy_sum, one scaling per kind), compose_reference's (reduced products
    per kind) and the statement's (sum of beta_q times quotient codeword q)"""
    for name in ROUTE_SETS:
        ops = Operands(shape, name)
        weights = cc.compose_weights(shape, ops)
        for params in ((ops.params, None) if shape.air.num_params else (ops.params,)):
            what = "%r %s%s" % (shape, name, "" if params is not None else " (params NULL)")
            lazy = (0, 0, 0)
            for kind, streams in cc.kind_streams(shape, ops, weights, params):
                values = tuple(np.array(l, dtype=object) for l in cc.reduce_streams(streams)[0])
                lazy = xadd(lazy, xscale(values, shape.zerofier[kind]))
            stated = (0, 0, 0)
            for beta, q in zip(weights, quotients(shape, ops, cc.NO_PARAMS if params is None else params)):
                stated = xadd(stated, xmul(beta, q))
            want = cc.compose_reference(shape, ops, weights, params, 0, None)
            same(lazy, want, what + ": unreduced sums")
            same(stated, want, what + ": weighted quotient codewords")
            for log_step in (1, 2, LOG_N):
                seeded = [l[::1 << log_step] for l in ops.seeded]
                stepped = cc.compose_reference(shape, ops, weights, params, log_step, seeded)
                same(stepped, [(w[::1 << log_step] + s) % P for w, s in zip(want, seeded)], what + ": log_step %d" % log_step)
                assert len(stepped[0]) == N >> log_step


def test_the_reference_on_chosen_rows_is_the_reference():
    rows = [0, 1, 7, 255, 256, 300, 504, 511]
    for shape in (SHAPES[0], SHAPES[2], SHAPES[4], cc.COMPOSE_SHAPES[7], cc.COMPOSE_SHAPES[11]):
        ops = Operands(shape, "random")
        weights = cc.compose_weights(shape, ops)
        want = cc.compose_reference(shape, ops, weights, ops.params, 0, None)
        got = cc.compose_reference_rows(shape.table, LOG_N, OFFSET, shape.height, ops.base, ops.ext, ops.challenges, ops.terminals, ops.params, weights, rows)
        same(got, [l[rows] for l in want], repr(shape))


def test_the_difference_reference_is_the_weighted_difference_quotient():
    from pointwise_cases import POINTS, difference_operands, inverse
    lhs, rhs, acc = difference_operands()
    weight = (fs.PALETTE[3], fs.PALETTE[14], fs.PALETTE[8])
    got = cc.difference_reference(lhs, rhs, weight, 1, [l[::2] for l in acc])
    for k in (0, 1, 100, 255):
        i = 2 * k
        q = tuple((int(a[i]) - int(b[i])) * inverse(POINTS[i] - 1) % P for a, b in zip(lhs, rhs))
        assert tuple(int(l[k]) for l in got) == xadd(tuple(int(l[i]) for l in acc), xmul(weight, q))


def test_extension_valued_quotients_are_the_generated_headers():
    generated = cc.generated_q_ext()
    assert sorted(generated) == sorted(a.name for a in air.TABLE_AIRS)
    for table, a in enumerate(air.TABLE_AIRS):
        assert cc.q_ext(table) == generated[a.name], a.name
    # the boundary kinds the planted launches aim at: 5 base cells and 2 extension cells (11 products per limb), 3 base cells (3)
    assert cc.q_ext(0)[:7] == (False,) * 5 + (True,) * 2 and cc.q_ext(2)[:3] == (False,) * 3


def test_kind_streams_takes_one_weight_per_quotient():
    counts = cc.generated_num_quotients()
    for shape in SHAPES[:4] + SHAPES[5:6]:
        nq = sum(len(constraints) for _, constraints in air.TABLE_AIRS[shape.table].all())
        assert nq == shape.nq == counts[shape.air.name] == len(cc.q_ext(shape.table))
        ops = Operands(shape, "cycling")
        weights = cc.compose_weights(shape, ops)
        streams = cc.kind_streams(shape, ops, weights, ops.params)
        assert [kind for kind, _ in streams] == list(cc.KINDS)
        products = sum(3 if e else 1 for e in cc.q_ext(shape.table))
        assert [sum(len(s[l]) for _, s in streams) for l in range(3)] == [products] * 3
        for wrong in (weights[:-1], weights + [weights[0]]):
            with pytest.raises(AssertionError):
                cc.kind_streams(shape, ops, wrong, ops.params)
    assert counts == {"processor": 21, "instruction": 10, "memory": 11, "input": 3, "output": 3}


def test_planted_launches_reach_the_boundary_floors():
    """the memory table's search run again; the processor table's pinned seeds checked"""
    kept, acc, inner = cc.planted_search(2)
    assert kept == cc.PLANTED_SEEDS[2]
    for table in cc.PLANTED_TABLES:
        if table != 2:
            acc, inner = set(), set()
            for ops in cc.planted_launches(table):
                a, r = cc.boundary_states(ops)
                assert (a - acc) or (r - inner), "launch %s of table %d adds no state" % (ops.name, table)
                acc |= a
                inner |= r
        want_acc, want_inner = cc.BOUNDARY_FLOOR[table]
        assert want_acc <= acc, (table, sorted(want_acc - acc))
        assert want_inner <= inner, (table, sorted(want_inner - inner))
    assert cc.BOUNDARY_FLOOR[0] == (fs.ACC_REQUIRED, fs.ACC_INNER_REQUIRED)
    assert cc.BOUNDARY_FLOOR[2] == (fs.ACC_REQUIRED - cc.MEMORY_UNREACHED, fs.ACC_INNER_REQUIRED) and cc.MEMORY_UNREACHED < fs.ACC_REQUIRED
    # a witness row holds the witness's operands and nothing else in its boundary cells
    ops = cc.designed_launch(0)
    wide = fs.ACC_WITNESSES[(1, 1, 0, 1, 0)]
    cells = cc.boundary_cells(ops.shape, ops)
    assert [int(cell[fs.WITNESS_ROWS[0]]) for cell, _ in cells] == [a for a, _ in wide] + [0] * (len(cells) - len(wide))
    assert [beta[0] for beta in cc.compose_weights(ops.shape, ops)[:len(wide)]] == [b for _, b in wide]


def test_the_other_sums_reach_what_is_pinned():
    reached = cc.reached_states()
    assert sorted(cc.REACHED) == sorted(k for k in reached if not (k[0] in cc.PLANTED_TABLES and k[1] == "boundary"))
    for key, (acc, inner) in cc.REACHED.items():
        assert acc <= reached[key][0], (key, sorted(acc - reached[key][0]))
        assert inner <= reached[key][1], (key, sorted(inner - reached[key][1]))
        assert acc <= set(fs.ACC_REQUIRED) | set(fs.ACC_NO_WITNESS) and inner <= fs.ACC_INNER_REQUIRED
    for table in cc.PLANTED_TABLES:
        want_acc, want_inner = cc.BOUNDARY_FLOOR[table]
        assert want_acc <= reached[table, "boundary"][0] and want_inner <= reached[table, "boundary"][1]
