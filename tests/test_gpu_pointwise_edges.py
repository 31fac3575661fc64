"""The pointwise kernels of the prover (csrc/air.hip) on codewords, challenges, terminals and weights of the test's own choosing,
through the C ABI and without a trace: palette values (tests/field_states.py) in every cell and scalar, challenges of zero and of
p - 1, random residues, and launches planted so that the unreduced column sums of the combination go through every required carry
state.  The reference is stark_brainfuck_amd/air.py evaluated on Python integers (object arrays: all 512 rows per call of
air.evaluate), the zerofier inverses and the weighted sum taken in Python; every comparison is exact and every word must be < p."""
import ctypes
import functools

import numpy as np
import pytest

import field_states as fs
from pointwise_cases import (HEIGHT, LOG_N, N, OFFSET, OMEGA, PALETTE, POINTS, SETS, SHAPES, Operands, Shape, assert_codeword, difference_operands, full,
                             inverses, quotients, to_words)
from stark_brainfuck_amd.air import xadd, xmul, xscale

pytestmark = pytest.mark.gpu

P = fs.P
u64 = ctypes.c_uint64
WINDOW = (250, 12)                    # rows 250..261: crosses the edge between the two workgroups


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from stark_brainfuck_amd import _lib
    return _lib.load()            # raises BackendUnavailable if the HIP library is missing: no fallback


def ok(rc):
    from stark_brainfuck_amd import _lib
    _lib.check(rc)


def upload(values):
    from stark_brainfuck_amd.device import DeviceBuffer
    return DeviceBuffer.from_numpy(to_words(values))


def painted(count):
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer
    buf = DeviceBuffer(count)
    ok(_lib.load().bfs_memset(buf.ptr, 0xA5, 8 * count, 0))
    return buf


def download(buf, shape):
    from stark_brainfuck_amd.device import synchronize
    synchronize(0)
    return buf.to_numpy().reshape(shape)


def flat(triples):
    return (u64 * (3 * len(triples)))(*[int(v) for t in triples for v in t])


# ------------------------------------------------------------------------------------------------ the combination
def shifts_for(shape, pattern):
    """generic: one shift per kind of term (all columns, all boundary, all transition, all terminal quotients), which every run of
    the grouped kernel accepts -- one of them past n, so that the exponent i * shift is reduced mod n; ungrouped: every term its own"""
    if pattern == "ungrouped":
        return [1 + 37 * k for k in range(shape.nterm)]
    per_kind = [3] * (shape.bw + shape.xw)
    for (_, count), s in zip(shape.kinds, (7, N + 3, 2)):
        per_kind += [s] * count
    return per_kind


def combination(shape, ops, terms, shifts, start):
    """start + sum over the terms (base columns, extension columns, quotients) of (wa + wb x^shift) * value"""
    acc, powers = start, {}
    for (wa, wb), v, s in zip(ops.weights, terms, shifts):
        if s not in powers:
            powers[s] = np.array([pow(int(x), s, P) for x in POINTS], dtype=object)
        acc = xadd(acc, xmul(xadd(wa, xscale(wb, powers[s])), v))
    return tuple(full(l) for l in acc)


class Case:
    """reference and device buffers of one (shape, operand set), made once and shared by the variants"""

    def __init__(self, shape, ops, params_given):
        self.shape, self.ops = shape, ops
        self.params = ops.params if params_given else None
        self.quotients = quotients(shape, ops, ops.params if params_given else (1, 0, 0))
        self.terms = [(c, 0, 0) for c in ops.base] + list(ops.ext) + self.quotients
        self.d_base, self.d_ext = upload(ops.base), upload(ops.ext)
        self.d_randomizer = upload(ops.randomizer)
        self.ch, self.tm = flat(ops.challenges), flat(ops.terminals)
        self.pr = flat([self.params]) if params_given else None

    def air_args(self):
        s = self.shape
        return (LOG_N, s.unit_distance, s.height, s.omicron_inv, OFFSET, OMEGA, self.ch, self.tm, self.pr)

    def weight_array(self, shifts):
        from stark_brainfuck_amd import _lib
        ws = (_lib.CombWeight * self.shape.nterm)()
        for w, (wa, wb), s in zip(ws, self.ops.weights, shifts):
            w.wa, w.wb, w.shift = (u64 * 3)(*wa), (u64 * 3)(*wb), s
        return ws


def zerofier_inverse_codewords(lib, shape):
    """bfs_zerofier_inverses as table.zerofier_inverses asks for them -> (buffer, three device addresses)"""
    specs = [(0, 1), (0, shape.omicron_inv)] + ([(1, shape.log_height)] if shape.height else [])
    out = painted(len(specs) * N)
    ok(lib.bfs_zerofier_inverses(LOG_N, OFFSET, OMEGA, len(specs), (ctypes.c_uint32 * len(specs))(*[s[0] for s in specs]),
                                 (u64 * len(specs))(*[s[1] for s in specs]), out.ptr, 0))
    return out, (ctypes.c_void_p * 3)(out.ptr, out.ptr + 8 * N, out.ptr + 16 * N if shape.height else None)


def check_case(lib, case):
    from stark_brainfuck_amd import _lib
    shape, ops = case.shape, case.ops
    what = "%r %s%s" % (shape, ops.name, "" if case.pr is not None else " (params NULL)")
    # quotient codewords
    d_quotients = painted(3 * shape.nq * N)
    ok(lib.bfs_air_quotients(shape.table, case.d_base.ptr, case.d_ext.ptr, d_quotients.ptr, *case.air_args(), 0))
    assert_codeword(download(d_quotients, (3 * shape.nq, N)), [l for q in case.quotients for l in q], what + ": quotients")
    # the combined path: accumulator from the randomizer or onto seeded residues, zerofier inverses handed in or computed, both kernels
    inv_buffer, inv_ptrs = zerofier_inverse_codewords(lib, shape)
    want = {}
    for pattern in ("generic", "ungrouped"):
        shifts = shifts_for(shape, pattern)
        ws = case.weight_array(shifts)
        for start in ("randomizer", "seeded"):
            begin = xmul(ops.w0, ops.randomizer) if start == "randomizer" else ops.seeded
            want[pattern, start] = combination(shape, ops, case.terms, shifts, begin)
            for given in (True, False):
                d_acc = painted(3 * N) if start == "randomizer" else upload(ops.seeded)
                ok(lib.bfs_air_combine(shape.table, case.d_base.ptr, case.d_ext.ptr, *case.air_args(), ws,
                                       case.d_randomizer.ptr if start == "randomizer" else None, flat([ops.w0]) if start == "randomizer" else None,
                                       d_acc.ptr, inv_ptrs if given else None, 0))
                assert_codeword(download(d_acc, (3, N)), want[pattern, start],
                                "%s: combine, %s shifts, from %s, inverses %s" % (what, pattern, start, "given" if given else "computed"))
    # a window of rows that crosses the workgroup edge: the rows inside move, the others keep their seeded residues
    first, count = WINDOW
    shifts = shifts_for(shape, "generic")
    d_acc = upload(ops.seeded)
    ok(lib.bfs_air_combine_rows(shape.table, case.d_base.ptr, case.d_ext.ptr, *case.air_args(), case.weight_array(shifts), None, None, d_acc.ptr,
                                inv_ptrs, first, count, 0))
    inside = np.arange(N)
    inside = (inside >= first) & (inside < first + count)
    assert_codeword(download(d_acc, (3, N)), [np.where(inside, new, old) for new, old in zip(want["generic", "seeded"], ops.seeded)],
                    what + ": combine_rows %r" % (WINDOW,))
    # the written-out path: bfs_combination over the column codewords and the quotient codewords bfs_air_quotients wrote
    for pattern in ("generic", "ungrouped"):
        shifts = shifts_for(shape, pattern)
        sources = (_lib.CombSource * shape.nterm)()
        where = [(case.d_base.ptr + 8 * N * c, 0) for c in range(shape.bw)] + [(case.d_ext.ptr + 24 * N * c, 1) for c in range(shape.xw)]
        where += [(d_quotients.ptr + 24 * N * q, 1) for q in range(shape.nq)]
        for src, (ptr, is_ext), (wa, wb), s in zip(sources, where, ops.weights, shifts):
            src.ptr, src.is_ext, src.pad, src.shift, src.wa, src.wb = ptr, is_ext, 0, s, (u64 * 3)(*wa), (u64 * 3)(*wb)
        d_out = painted(3 * N)
        ok(lib.bfs_combination(sources, shape.nterm, case.d_randomizer.ptr, flat([ops.w0]), d_out.ptr, LOG_N, OFFSET, OMEGA, 0))
        assert_codeword(download(d_out, (3, N)), want[pattern, "randomizer"], "%s: bfs_combination, %s shifts" % (what, pattern))
    del inv_buffer


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("shape", SHAPES, ids=repr)
def test_quotients_and_combination_on_chosen_codewords(lib, shape, name):
    ops = Operands(shape, name)
    check_case(lib, Case(shape, ops, params_given=True))
    if shape.air.num_params:          # the tables that read h_params: NULL stands for 1
        check_case(lib, Case(shape, ops, params_given=False))


# ------------------------------------------------------------------------------------------------ planted launches
@functools.lru_cache(maxsize=None)
def planted_states():
    """the model's states over every table's planted launches (column weights only: wb = 0 and zero quotient weights keep the
    accumulator of the column kind equal to the modelled stream)"""
    acc, inner = set(), set()
    for table in range(5):
        for launch in fs.planted_launches(table, N):
            a, r = fs.launch_states(launch, N)
            acc |= a
            inner |= r
    return acc, inner


@pytest.mark.parametrize("table", range(5))
def test_planted_launches_reach_every_required_accumulator_state(lib, table):
    assert N == fs.PLANTED_ROWS
    acc, inner = planted_states()
    assert fs.ACC_REQUIRED <= acc, sorted(fs.ACC_REQUIRED - acc)
    assert fs.ACC_INNER_REQUIRED <= inner, sorted(fs.ACC_INNER_REQUIRED - inner)
    shape = Shape(table, HEIGHT)
    for number, (weights, base, ext) in enumerate(fs.planted_launches(table, N)):
        ops = Operands(shape, "random")
        ops.base = [np.array(c, dtype=object) for c in base]
        ops.ext = [tuple(np.array(l, dtype=object) for l in c) for c in ext]
        ops.weights = [(w, (0, 0, 0)) for w in weights] + [((0, 0, 0), (0, 0, 0))] * shape.nq
        case = Case.__new__(Case)
        case.shape, case.ops, case.params = shape, ops, ops.params
        case.d_base, case.d_ext, case.d_randomizer = upload(ops.base), upload(ops.ext), upload(ops.randomizer)
        case.ch, case.tm, case.pr = flat(ops.challenges), flat(ops.terminals), flat([ops.params])
        columns = [(c, 0, 0) for c in ops.base] + list(ops.ext)
        total = (0, 0, 0)
        for w, v in zip(weights, columns):
            total = xadd(total, xmul(w, v))
        for pattern in ("generic", "ungrouped"):
            ws = case.weight_array(shifts_for(shape, pattern))
            for start in ("randomizer", "seeded"):
                begin = xmul(ops.w0, ops.randomizer) if start == "randomizer" else ops.seeded
                d_acc = painted(3 * N) if start == "randomizer" else upload(ops.seeded)
                ok(lib.bfs_air_combine(table, case.d_base.ptr, case.d_ext.ptr, *case.air_args(), ws,
                                       case.d_randomizer.ptr if start == "randomizer" else None, flat([ops.w0]) if start == "randomizer" else None,
                                       d_acc.ptr, None, 0))
                assert_codeword(download(d_acc, (3, N)), xadd(begin, total),
                                "%r planted launch %d, %s shifts, from %s" % (shape, number, pattern, start))


# ------------------------------------------------------------------------------------------------ difference quotients
def test_difference_quotient_on_palette_operands(lib):
    lhs, rhs, _ = difference_operands()
    assert {(int(a), int(b)) for a, b in zip(lhs[0], rhs[0])} == set(fs.palette_pairs())
    want = xscale(tuple((a - b) % P for a, b in zip(lhs, rhs)), inverses(POINTS - 1))
    d_lhs, d_rhs, d_out = upload(lhs), upload(rhs), painted(3 * N)
    ok(lib.bfs_difference_quotient(d_lhs.ptr, d_rhs.ptr, d_out.ptr, LOG_N, OFFSET, OMEGA, 0))
    assert_codeword(download(d_out, (3, N)), want, "difference quotient")


@pytest.mark.parametrize("k", range(len(PALETTE)))
def test_difference_combine_on_palette_operands(lib, k):
    """acc + (wa + wb x^shift) (lhs - rhs) / (x - 1) with every word of wa and wb one palette value; 1 / (x - 1) handed in and
    computed; the whole domain and a window across the workgroup edge"""
    from stark_brainfuck_amd import _lib
    lhs, rhs, acc = difference_operands()
    value = PALETTE[k]
    wa, wb = (value, PALETTE[(k + 1) % len(PALETTE)], value), (PALETTE[(k + 2) % len(PALETTE)], value, value)
    boundary = inverses(POINTS - 1)
    quotient = xscale(tuple((a - b) % P for a, b in zip(lhs, rhs)), boundary)
    d_lhs, d_rhs, d_inv = upload(lhs), upload(rhs), upload(boundary)
    for shift in (5, N + 3):
        weight = _lib.CombWeight((u64 * 3)(*wa), (u64 * 3)(*wb), shift)
        power = np.array([pow(int(x), shift, P) for x in POINTS], dtype=object)
        want = xadd(acc, xmul(xadd(wa, xscale(wb, power)), quotient))
        for given in (True, False):
            d_acc = upload(acc)
            ok(lib.bfs_difference_combine(d_lhs.ptr, d_rhs.ptr, LOG_N, OFFSET, OMEGA, ctypes.byref(weight), d_acc.ptr, d_inv.ptr if given else None, 0))
            assert_codeword(download(d_acc, (3, N)), want, "difference combine, palette %d, shift %d, inverse %s" % (k, shift, given))
        first, count = WINDOW
        d_acc = upload(acc)
        ok(lib.bfs_difference_combine_rows(d_lhs.ptr, d_rhs.ptr, LOG_N, OFFSET, OMEGA, ctypes.byref(weight), d_acc.ptr, d_inv.ptr, first, count, 0))
        inside = np.arange(N)
        inside = (inside >= first) & (inside < first + count)
        assert_codeword(download(d_acc, (3, N)), [np.where(inside, new, old) for new, old in zip(want, acc)],
                        "difference combine rows, palette %d, shift %d" % (k, shift))
