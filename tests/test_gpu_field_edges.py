"""The field primitives on operands chosen for the carries they go through (tests/field_states.py): the witness pairs of the fused
product's rare states, every pair of palette values and 2^12 random pairs, through every entry point that multiplies -- compared
word for word with Python integers.  tests/test_field_states_host.py asserts which states these operands reach."""
import ctypes
import random

import numpy as np
import pytest

import field_states as fs

pytestmark = pytest.mark.gpu

P = fs.P
RANDOM_PAIRS = 1 << 12
BFS_ERR_BAD_ARG = 6
RAGGED = 2048 + 3                    # one past eight full workgroups, and odd


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from stark_brainfuck_amd import _lib
    return _lib.load()            # raises BackendUnavailable if the HIP library is missing: no fallback


@pytest.fixture(scope="module")
def pairs():
    """edge pairs first (witnesses, search results, palette pairs, both orders), then the random ones"""
    edge = fs.fused_operands()
    assert fs.FUSED_REQUIRED <= fs.fused_states(edge)
    return edge, edge + fs.random_pairs(RANDOM_PAIRS, seed=0xED6E)


def ok(rc):
    from stark_brainfuck_amd import _lib
    _lib.check(rc)


def sync():
    from stark_brainfuck_amd.device import synchronize
    synchronize(0)


def upload(values):
    from stark_brainfuck_amd.device import DeviceBuffer
    return DeviceBuffer.from_numpy(np.array(values, dtype=np.uint64).reshape(-1))


def empty(count):
    from stark_brainfuck_amd.device import DeviceBuffer
    buf = DeviceBuffer(count)
    ok(library().bfs_memset(buf.ptr, 0xA5, 8 * count, 0))
    return buf


def library():
    from stark_brainfuck_amd import _lib
    return _lib.load()


def words(buf, count=None):
    sync()
    return [int(v) for v in buf.to_numpy(count)]


def first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return i
    return None


def test_gl_mul_pointwise_on_chosen_pairs(lib, pairs):
    _, every = pairs
    a, b = upload([p[0] for p in every]), upload([p[1] for p in every])
    want = [x * y % P for x, y in every]
    for n in (len(every), RAGGED):
        out = empty(n)
        ok(lib.bfs_gl_mul_pointwise(a.ptr, b.ptr, out.ptr, n, 0))
        got = words(out)
        bad = first_difference(got, want[:n])
        assert bad is None, "n = %d, pair %d: %x * %x gives %x, expected %x" % (n, bad, *every[bad], got[bad], want[bad])


def test_xfe_mul_pointwise_with_the_pairs_in_every_limb_position(lib, pairs):
    """element (pair, la, lb): limb la of the first operand is the pair's a, limb lb of the second its b, the other four limbs seeded
    residues -- each of the nine products of the schoolbook multiplication sees every edge pair"""
    edge, _ = pairs
    rng = random.Random(0x11B)
    xs, ys = [], []
    for a, b in edge:
        for la in range(3):
            for lb in range(3):
                x, y = [rng.randrange(P) for _ in range(3)], [rng.randrange(P) for _ in range(3)]
                x[la], y[lb] = a, b
                xs.append(tuple(x))
                ys.append(tuple(y))
    for _ in range(RANDOM_PAIRS):
        xs.append(tuple(rng.randrange(P) for _ in range(3)))
        ys.append(tuple(rng.randrange(P) for _ in range(3)))
    total = len(xs)
    assert total % 256 != 0
    want = [fs._xmul(x, y) for x, y in zip(xs, ys)]
    planes = lambda elements: upload([[e[l] for e in elements] for l in range(3)])
    a, b = planes(xs), planes(ys)
    for n in (total, RAGGED):
        out = empty(3 * total)
        ok(lib.bfs_xfe_mul_pointwise(a.ptr, total, b.ptr, total, out.ptr, total, n, 0))
        got = np.array(words(out), dtype=object).reshape(3, total)
        for i in range(n):
            assert tuple(got[:, i]) == want[i], "n = %d, element %d: %s * %s gives %s, expected %s" % (n, i, xs[i], ys[i], tuple(got[:, i]), want[i])
        assert all(v == 0xA5A5A5A5A5A5A5A5 for v in got[:, n:].reshape(-1)), "n = %d: words past the end were written" % n


def test_gl_scale_with_the_pairs_first_operand_as_the_factor(lib, pairs):
    """bfs_gl_scale multiplies element i by factor^i: one call per distinct first operand a, one row of four elements per pair
    (a, b) with b at index 1 -- the product b * a itself -- and seeded residues at 0, 2 and 3"""
    edge, _ = pairs
    rng = random.Random(0x5CA1E)
    by_factor = {}
    for a, b in edge:
        by_factor.setdefault(a, []).append(b)
    assert len(by_factor) < 64
    n, stride = 4, 5
    for factor, seconds in sorted(by_factor.items()):
        rows = [[rng.randrange(P), b, rng.randrange(P), rng.randrange(P), rng.randrange(P)] for b in seconds]
        src, out = upload(rows), empty(len(rows) * stride)
        ok(lib.bfs_gl_scale(src.ptr, out.ptr, n, stride, len(rows), factor, 0))
        got = np.array(words(out), dtype=object).reshape(len(rows), stride)
        for r, row in enumerate(rows):
            want = [row[i] * pow(factor, i, P) % P for i in range(n)]
            assert list(got[r, :n]) == want, "factor %x, row %d (%x): %s, expected %s" % (factor, r, row[1], list(got[r, :n]), want)
            assert got[r, n] == 0xA5A5A5A5A5A5A5A5


def test_gl_batch_inverse_multiplies_the_pairs(lib, pairs):
    """the kernel's thread t of a 2048-element block multiplies elements t, 256 + t, ... up: a at t and b at 256 + t make its
    first product a * b.  Pairs without a zero, 256 per block, seeded residues elsewhere, a ragged last block."""
    edge, _ = pairs
    rng = random.Random(0x1A7)
    planted = [(a, b) for a, b in edge if a and b]
    blocks = -(-len(planted) // 256)
    total = 2048 * blocks + RAGGED
    values = [rng.randrange(1, P) for _ in range(total)]
    for k, (a, b) in enumerate(planted):
        base = 2048 * (k // 256) + k % 256
        values[base], values[base + 256] = a, b
    values[2048 * blocks:2048 * blocks + len(fs.PALETTE) - 1] = [v for v in fs.PALETTE if v]
    want = [pow(v, P - 2, P) for v in values]
    src = upload(values)
    for n in (total, RAGGED):
        out = empty(n)
        ok(lib.bfs_gl_batch_inverse(src.ptr, out.ptr, n, 0))
        got = words(out)
        bad = first_difference(got, want[:n])
        assert bad is None, "n = %d, element %d: 1 / %x gives %x, expected %x" % (n, bad, values[bad], got[bad], want[bad])


def test_selftest_field_pairs_against_python_integers(lib, pairs):
    """the 50 operations of csrc/selftest.hip on the chosen pairs, raw device words against their restatement in Python integers:
    operations 0..41, 45, 46, 48 and 49 are canonical and compared exactly; 42, 43, 44 and 47 may be unreduced and are compared as
    residues -- and exactly against the unreduced sum's own definition (a + b mod 2^64, + 2^32 - 1 when that wrapped)"""
    _, every = pairs
    n = len(every)
    flat = np.array(every, dtype=np.uint64).reshape(-1)
    out = np.full(fs.SELFTEST_OPS * n, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    ok(lib.bfs_selftest_field_pairs(flat.ctypes.data, n, out.ctypes.data))
    got = out.reshape(n, fs.SELFTEST_OPS)

    def add_lazy(x, y):
        s = x + y
        return (s + fs.EPS) & fs.M64 if s >> 64 else s
    for i, (a, b) in enumerate(every):
        want = fs.selftest_reference(a, b)
        row = [int(v) for v in got[i]]
        for j in range(fs.SELFTEST_OPS):
            if j in fs.SELFTEST_LAZY:
                assert row[j] % P == want[j], "operation %d on a=%x b=%x: %x, expected a value congruent to %x" % (j, a, b, row[j], want[j])
            else:
                assert row[j] == want[j], "operation %d on a=%x b=%x: %x, expected %x" % (j, a, b, row[j], want[j])
        lazy, anything = add_lazy(a, b), ~a & fs.M64
        assert row[42] == lazy and row[43] == add_lazy(lazy, (a - b) % P) and row[47] == add_lazy(anything, b), (hex(a), hex(b))
    # an operand >= p is refused before anything runs
    refused = np.array([1, P], dtype=np.uint64)
    before = out.copy()
    assert lib.bfs_selftest_field_pairs(refused.ctypes.data, 1, out.ctypes.data) == BFS_ERR_BAD_ARG
    assert (out == before).all()
    # and the comparing entry still runs on the same kernel
    bad = ctypes.c_uint64(1)
    ok(lib.bfs_selftest_field(12, ctypes.byref(bad)))
    assert bad.value == 0, lib.bfs_last_error().decode()
