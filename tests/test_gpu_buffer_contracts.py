"""What every device-writing entry point of include/bfstark.h does to memory that is NOT its result, and what it does when its
output aliases an input.  Each case asserts four things:
  * values: exact against oracle.*, hashlib or the host primitive the entry's own parity test uses;
  * containment: the output lies in a painted arena (tests/painted.py: guards of 4096 words, small odd gaps inside a batch) and
    nothing outside the result ranges changes;
  * inputs: every input buffer of an out-of-place call reads back as it went up;
  * aliasing: every aliasing mode the header allows gives the out-of-place values.
Every access of every test lies inside an allocation the test made.  Sizes are the smallest that take each launch shape."""
import ctypes
import functools
import hashlib
import random

import numpy as np
import pytest

import commitment_check as cc
import fri_coset_model as coset_model
import fri_folding_model as folding_model
from painted import PAINT_BYTE, PAINT_WORD, Arena, Layout, Violation
from stream_builders import PAD_MASKS, PAD_WIDTH, padded, strided

pytestmark = pytest.mark.gpu

SEED = 0xA11A5
P = (1 << 64) - (1 << 32) + 1
OFFSET = 7
BFS_ERR_ZERO_IN_BATCH_INVERSE, BFS_ERR_BAD_ARG = 5, 6
u64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def sb():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import stark_brainfuck_amd
    from stark_brainfuck_amd import _lib
    _lib.load()            # raises BackendUnavailable if the HIP library is missing: no fallback
    return stark_brainfuck_amd


@pytest.fixture(scope="module")
def lib(sb):
    from stark_brainfuck_amd import _lib
    return _lib.load()


def ok(rc):
    from stark_brainfuck_amd import _lib
    _lib.check(rc)


def sync():
    from stark_brainfuck_amd.device import synchronize
    synchronize(0)


class Input:
    """an input buffer of a call: uint64 words (or bytes, padded to whole words) in HBM and the host copy that went up"""

    def __init__(self, name, host):
        from stark_brainfuck_amd.device import DeviceBuffer
        host = np.ascontiguousarray(host)
        assert host.dtype in (np.dtype(np.uint64), np.dtype(np.uint8))
        self.name, self.dtype, self.size = name, host.dtype, host.size
        raw = host.reshape(-1).view(np.uint8)
        padded = np.zeros(-(-max(raw.size, 8) // 8) * 8, dtype=np.uint8)
        padded[:raw.size] = raw
        self.host = padded.view(np.uint64).copy()
        self.buf = DeviceBuffer.from_numpy(self.host)
        self.ptr = self.buf.ptr

    def address(self, offset):
        return self.ptr + int(offset) * self.dtype.itemsize

    def after(self):
        """(name, before, after) for the checker"""
        return (self.name, self.host, self.buf.to_numpy())


def residues(oracle, seed, count):
    return oracle.felt_array(SEED + seed, 0, count)


def nonzero(a):
    return np.where(a == 0, np.uint64(1), a)


# ------------------------------------------------------------------------------------------------ the checker on real buffers
def test_the_checker_flags_one_guard_word_set_on_the_device(lib):
    """a single bfs_memset of one guard word, inside the allocation: the arena read back from HBM fails the check, in the region and
    at the offset that were hit; the untouched arena passes"""
    arena = Arena(batch=3, stride=24, n=17)
    assert arena.contained() is not None
    assert (arena.snapshot() == np.uint64(PAINT_WORD)).all()
    for region, start, offset in (("back guard", arena.layout.guard + 3 * 24, 5), ("gap 1", arena.layout.guard + 24 + 17, 6), ("front guard", 0, 4095)):
        fresh = Arena(batch=3, stride=24, n=17)
        ok(lib.bfs_memset(fresh.buf.ptr + 8 * (start + offset), 0, 8, 0))
        sync()
        with pytest.raises(Violation) as e:
            fresh.contained()
        assert (e.value.region, e.value.offset, e.value.before, e.value.after) == (region, offset, PAINT_WORD, 0)
    octets = Arena(batch=1, stride=100, n=100, dtype=np.uint8)
    ok(lib.bfs_memset(octets.address(100), 0, 1, 0))
    sync()
    with pytest.raises(Violation) as e:
        octets.contained()
    assert (e.value.region, e.value.offset, e.value.before) == ("back guard", 0, PAINT_BYTE)


# ------------------------------------------------------------------------------------------------ bfs_gl_ntt
def ntt_want(oracle, coeffs, n, shift, scale):
    w = oracle.primitive_nth_root(n)
    out = oracle.fast_coset_evaluate(coeffs, shift, w, n)
    return out if scale == 1 else oracle.hadamard(out, np.full(n, scale, dtype=np.uint64))


def ntt_fills(logn):
    n = 1 << logn
    fills = {n, n // 4 + 1}
    if logn in (13, 16, 17):
        fills.add(n // 16)                  # the expansion plan (PASS_EXPAND)
    return sorted(f for f in fills if 1 <= f <= n)


@pytest.mark.parametrize("logn,n_in", [(logn, f) for logn in list(range(14)) + [16, 17] for f in ntt_fills(logn) if logn <= 13 or f == (1 << logn) // 16])
def test_ntt_writes_its_transforms_and_nothing_else(lib, oracle, logn, n_in):
    """the small kernel (2^0 .. 2^3), the single pass (2^4 .. 2^12), the first multi-pass size and the expansion plan: batch 3,
    in_stride = n_in + 5, out_stride = n + 3, coset shift 7, post-scale n^-1.  The gaps of the input hold residues that no transform
    may read as coefficients (the values would differ)."""
    n, batch = 1 << logn, 3
    in_stride, out_stride = n_in + 5, n + 3
    w, scale = oracle.primitive_nth_root(n), oracle.inv(n)
    src = Input("coefficients", residues(oracle, 100 * logn + n_in % 97, batch * in_stride))
    out = Arena(batch=batch, stride=out_stride, n=n)
    ok(lib.bfs_gl_ntt(src.ptr, n_in, in_stride, out.ptr, out_stride, logn, batch, w, 7, scale, 0))
    sync()
    after = out.contained([src.after()])
    got = out.rows(after)
    for b in range(batch):
        assert (got[b] == ntt_want(oracle, src.host[b * in_stride:b * in_stride + n_in], n, 7, scale)).all(), b


@pytest.mark.parametrize("logn", list(range(14)))
def test_ntt_in_place_with_equal_strides(lib, oracle, logn):
    """aliasing (a): d_in == d_out, in_stride == out_stride, batch 3 -- every transform overwrites its own input only"""
    n, batch = 1 << logn, 3
    stride = n + 3
    w, scale = oracle.primitive_nth_root(n), oracle.inv(n)
    cols = residues(oracle, 200 + logn, batch * n).reshape(batch, n)
    arena = Arena(batch=batch, stride=stride, n=n)
    arena.fill_rows(cols)
    ok(lib.bfs_gl_ntt(arena.ptr, n, stride, arena.ptr, stride, logn, batch, w, 7, scale, 0))
    sync()
    got = arena.rows(arena.contained())
    for b in range(batch):
        assert (got[b] == ntt_want(oracle, cols[b], n, 7, scale)).all(), b


@pytest.mark.parametrize("logn", list(range(2, 13)))
def test_ntt_output_that_starts_inside_its_input(lib, oracle, logn):
    """aliasing (b): one zero-padded transform of n / 4 coefficients whose output starts in the middle of them.  The first half of
    the coefficients lies in front of the output and is not written."""
    n = 1 << logn
    d = n // 4
    w = oracle.primitive_nth_root(n)
    coeffs = residues(oracle, 300 + logn, d)
    arena = Arena(Layout(results=[(d // 2, n)], payload=d // 2 + n))
    arena.fill(0, coeffs)
    ok(lib.bfs_gl_ntt(arena.ptr, d, d, arena.address(d // 2), n, logn, 1, w, 7, 1, 0))
    sync()
    after = arena.contained()
    assert (arena.layout.result(after) == ntt_want(oracle, coeffs, n, 7, 1)).all()


def ntt_workgroups_resident(logn):
    """an upper bound on the workgroups of bfs_gl_ntt's one-workgroup-per-transform kernels the device holds at once: 32 waves per
    compute unit over the waves of a workgroup (the small kernel launches 64 threads, a single-pass tile n / 16 threads)"""
    import torch
    threads = 64 if logn <= 3 else max(1, (1 << logn) // 16)
    waves = -(-threads // 64)
    return (32 // waves) * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("logn", [3, 6, 10, 12, 13, 16])
def test_ntt_in_place_extension_of_a_packed_batch(lib, oracle, logn):
    """aliasing (c): d_in == d_out, n_in = in_stride = n / 4, out_stride = n -- output b covers the inputs of transforms 4b .. 4b + 3.
    The batch is at least four times what the device can hold at once (asserted), so that late workgroups start after early ones
    have stored; at 2^13 and 2^16 the route through the library buffer does not depend on residency and 64 transforms do.
    Expected values: the same call out of place, itself checked against the oracle on transforms 0, 1, the last and 64 seeded ones
    (three quarters of them from the upper three quarters of the batch); in place must equal it word for word."""
    n = 1 << logn
    d = n // 4
    if logn <= 12:
        resident = ntt_workgroups_resident(logn)
        batch = min(65535, max({3: 65535, 6: 65535, 10: 16384, 12: 8192}[logn], 4 * resident))
        assert batch >= 4 * resident, "batch %d does not exceed four times the %d resident workgroups" % (batch, resident)
        assert batch * n * 8 <= 256 << 20
    else:
        batch = 64
    w = oracle.primitive_nth_root(n)
    coeffs = residues(oracle, 400 + logn, batch * d)
    src = Input("coefficients", coeffs)
    apart = Arena(batch=batch, stride=n, n=n)
    ok(lib.bfs_gl_ntt(src.ptr, d, d, apart.ptr, n, logn, batch, w, 7, 1, 0))
    sync()
    want = apart.contained([src.after()])
    rng = random.Random(logn)
    picks = [0, 1, batch - 1] + [rng.randrange(batch // 4, batch) for _ in range(48)] + [rng.randrange(0, max(batch // 4, 1)) for _ in range(16)]
    rows = apart.layout.payload_of(want).reshape(batch, n)
    for b in picks:
        assert (rows[b] == ntt_want(oracle, coeffs[b * d:(b + 1) * d], n, 7, 1)).all(), b
    inplace = Arena(batch=batch, stride=n, n=n)
    inplace.fill(0, coeffs)
    ok(lib.bfs_gl_ntt(inplace.ptr, d, d, inplace.ptr, n, logn, batch, w, 7, 1, 0))
    sync()
    got = inplace.contained()
    differ = np.flatnonzero(inplace.layout.payload_of(got) != apart.layout.payload_of(want))
    assert differ.size == 0, "%d words differ from the out-of-place call, first in transform %d at element %d" % (
        differ.size, differ[0] // n, differ[0] % n)


# ------------------------------------------------------------------------------------------------ element-wise entry points
ELEMENTWISE_SIZES = [1, 7, 2049, 524289]         # the last: one past 2048 workgroups of 256, where the grid-stride loop starts


@pytest.mark.parametrize("n", ELEMENTWISE_SIZES)
def test_gl_mul_pointwise(lib, oracle, n):
    a, b = residues(oracle, 1, n), residues(oracle, 2, n)
    da, db = Input("a", a), Input("b", b)
    out = Arena(batch=1, stride=n, n=n)
    ok(lib.bfs_gl_mul_pointwise(da.ptr, db.ptr, out.ptr, n, 0))
    sync()
    want = oracle.hadamard(a, b)
    assert (out.rows(out.contained([da.after(), db.after()]))[0] == want).all()
    for mode in ("out == a", "out == b"):
        arena = Arena(batch=1, stride=n, n=n)
        arena.fill(0, a if mode == "out == a" else b)
        other = Input("the other operand", b if mode == "out == a" else a)
        args = (arena.ptr, other.ptr) if mode == "out == a" else (other.ptr, arena.ptr)
        ok(lib.bfs_gl_mul_pointwise(args[0], args[1], arena.ptr, n, 0))
        sync()
        assert (arena.rows(arena.contained([other.after()]))[0] == want).all(), mode
    arena = Arena(batch=1, stride=n, n=n)
    arena.fill(0, a)
    ok(lib.bfs_gl_mul_pointwise(arena.ptr, arena.ptr, arena.ptr, n, 0))
    sync()
    assert (arena.rows(arena.contained())[0] == oracle.hadamard(a, a)).all(), "a == b == out"


@pytest.mark.parametrize("n", ELEMENTWISE_SIZES)
def test_gl_batch_inverse(lib, oracle, n):
    a = nonzero(residues(oracle, 3, n))
    da = Input("values", a)
    out = Arena(batch=1, stride=n, n=n)
    ok(lib.bfs_gl_batch_inverse(da.ptr, out.ptr, n, 0))
    want = oracle.batch_inverse(a)
    assert (out.rows(out.contained([da.after()]))[0] == want).all()
    arena = Arena(batch=1, stride=n, n=n)
    arena.fill(0, a)
    ok(lib.bfs_gl_batch_inverse(arena.ptr, arena.ptr, n, 0))
    assert (arena.rows(arena.contained())[0] == want).all(), "in place"
    # a zero element: the reference's assertion, zero in its place, the other inverses as before, the guards alone
    z = a.copy()
    z[n // 2] = 0
    dz = Input("values with a zero", z)
    out = Arena(batch=1, stride=n, n=n)
    assert lib.bfs_gl_batch_inverse(dz.ptr, out.ptr, n, 0) == BFS_ERR_ZERO_IN_BATCH_INVERSE
    got = out.rows(out.contained([dz.after()]))[0]
    keep = np.arange(n) != n // 2
    assert got[n // 2] == 0 and (got[keep] == want[keep]).all()


@pytest.mark.parametrize("n", ELEMENTWISE_SIZES)
def test_gl_scale(lib, oracle, n):
    """batch 3, stride n + 7"""
    batch, stride = 3, n + 7
    factor = int(residues(oracle, 4, 1)[0]) | 1
    cols = residues(oracle, 5, batch * n).reshape(batch, n)
    src = Input("coefficients", strided(cols, stride, residues(oracle, 6, batch * stride)))
    out = Arena(batch=batch, stride=stride, n=n)
    ok(lib.bfs_gl_scale(src.ptr, out.ptr, n, stride, batch, factor, 0))
    sync()
    want = np.stack([oracle.scale(factor, c) for c in cols])
    assert (out.rows(out.contained([src.after()])) == want).all()
    arena = Arena(batch=batch, stride=stride, n=n)
    arena.fill_rows(cols)
    ok(lib.bfs_gl_scale(arena.ptr, arena.ptr, n, stride, batch, factor, 0))
    sync()
    assert (arena.rows(arena.contained()) == want).all(), "in place"


def xfe_operands(oracle, n):
    a, b = residues(oracle, 7, 3 * n).reshape(3, n), residues(oracle, 8, 3 * n).reshape(3, n)
    b[0] = np.where((b[0] | b[1] | b[2]) == 0, np.uint64(1), b[0])
    return a, b


@pytest.mark.parametrize("n", ELEMENTWISE_SIZES)
def test_xfe_mul_pointwise(lib, oracle, n):
    """three different strides; out == a, out == b and a == b == out with the aliased operands' strides equal"""
    a, b = xfe_operands(oracle, n)
    sa, sb_, so = n + 1, n + 4, n + 9
    da = Input("a", strided(a, sa, residues(oracle, 9, 3 * sa)))
    db = Input("b", strided(b, sb_, residues(oracle, 10, 3 * sb_)))
    out = Arena(batch=3, stride=so, n=n)
    ok(lib.bfs_xfe_mul_pointwise(da.ptr, sa, db.ptr, sb_, out.ptr, so, n, 0))
    sync()
    want = oracle.xhadamard(a, b)
    assert (out.rows(out.contained([da.after(), db.after()])) == want).all()
    arena = Arena(batch=3, stride=so, n=n)
    arena.fill_rows(a)
    ok(lib.bfs_xfe_mul_pointwise(arena.ptr, so, db.ptr, sb_, arena.ptr, so, n, 0))
    sync()
    assert (arena.rows(arena.contained([db.after()])) == want).all(), "out == a"
    arena = Arena(batch=3, stride=so, n=n)
    arena.fill_rows(b)
    ok(lib.bfs_xfe_mul_pointwise(da.ptr, sa, arena.ptr, so, arena.ptr, so, n, 0))
    sync()
    assert (arena.rows(arena.contained([da.after()])) == want).all(), "out == b"
    arena = Arena(batch=3, stride=so, n=n)
    arena.fill_rows(a)
    ok(lib.bfs_xfe_mul_pointwise(arena.ptr, so, arena.ptr, so, arena.ptr, so, n, 0))
    sync()
    assert (arena.rows(arena.contained()) == oracle.xhadamard(a, a)).all(), "a == b == out"


@pytest.mark.parametrize("n", ELEMENTWISE_SIZES)
def test_xfe_batch_inverse(lib, oracle, n):
    _, b = xfe_operands(oracle, n)
    si, so = n + 2, n + 9
    db = Input("values", strided(b, si, residues(oracle, 11, 3 * si)))
    out = Arena(batch=3, stride=so, n=n)
    ok(lib.bfs_xfe_batch_inverse(db.ptr, si, out.ptr, so, n, 0))
    inv = out.rows(out.contained([db.after()]))
    if n <= 1 << 16:
        assert (inv == oracle.xbatch_inverse(b)).all()
    one = oracle.xhadamard(inv, b)            # the inverse is unique: inv * b == 1 pins every word
    assert (one[0] == 1).all() and not one[1:].any() and (inv < np.uint64(P)).all()
    arena = Arena(batch=3, stride=so, n=n)
    arena.fill_rows(b)
    ok(lib.bfs_xfe_batch_inverse(arena.ptr, so, arena.ptr, so, n, 0))
    assert (arena.rows(arena.contained()) == inv).all(), "in place"
    z = b.copy()
    z[:, n // 2] = 0
    dz = Input("values with a zero", strided(z, si, residues(oracle, 12, 3 * si)))
    out = Arena(batch=3, stride=so, n=n)
    assert lib.bfs_xfe_batch_inverse(dz.ptr, si, out.ptr, so, n, 0) == BFS_ERR_ZERO_IN_BATCH_INVERSE
    got = out.rows(out.contained([dz.after()]))
    keep = np.arange(n) != n // 2
    assert not got[:, n // 2].any() and (got[:, keep] == inv[:, keep]).all()


# ------------------------------------------------------------------------------------------------ subproduct tree
def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + int(c)) % P
    return acc


def distinct_points(rng, n):
    pts = set()
    while len(pts) < n:
        pts.add(rng.randrange(P))
    out = list(pts)
    rng.shuffle(out)
    return out


class Tree:
    """bfs_ptree_build over host points, freed on exit"""

    def __init__(self, lib, points):
        self.lib, self.points = lib, Input("points", np.array(points, dtype=np.uint64))
        self.handle = ctypes.c_void_p()
        ok(lib.bfs_ptree_build(self.points.ptr, len(points), 0, ctypes.byref(self.handle)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        ok(self.lib.bfs_ptree_free(self.handle, 0))
        sync()


@pytest.mark.parametrize("n", [1, 5, 64, 65, 1000])
def test_subproduct_tree_outputs(lib, n):
    """bfs_ptree_zerofier writes exactly n + 1 words; bfs_ptree_evaluate and bfs_ptree_interpolate with batch 3 and out_stride n + 5;
    points, coefficients and values are left alone.  Values against host arithmetic on Python integers, as in
    tests/test_gpu_subproduct.py: a monic polynomial of degree n that vanishes on the n points is the zerofier; a polynomial of n
    coefficients is pinned by its values on the points (all of them up to n = 65, 48 seeded ones at n = 1000)."""
    rng = random.Random(SEED + n)
    pts = distinct_points(rng, n)
    samples = list(range(n)) if n <= 128 else rng.sample(range(n), 48)
    batch, out_stride = 3, n + 5
    with Tree(lib, pts) as tree:
        assert lib.bfs_ptree_size(tree.handle) == n
        zero = Arena(batch=1, stride=n + 1, n=n + 1)
        ok(lib.bfs_ptree_zerofier(tree.handle, zero.ptr, 0))
        sync()
        z = [int(v) for v in zero.rows(zero.contained([tree.points.after()]))[0]]
        assert z[-1] == 1 and all(v < P for v in z)
        assert all(horner(z, pts[i]) == 0 for i in samples)
        for r in (rng.randrange(P) for _ in range(4)):
            want = 1
            for x in pts:
                want = want * (r - x) % P
            assert horner(z, r) == want
        # evaluation: more coefficients than points, and fewer
        for m in (n + 1, max(n // 2, 1)):
            in_stride = m + 2
            coeffs = [[rng.randrange(P) for _ in range(m)] for _ in range(batch)]
            src = Input("coefficients", strided(np.array(coeffs, dtype=np.uint64), in_stride, np.arange(1, batch * in_stride + 1, dtype=np.uint64)))
            out = Arena(batch=batch, stride=out_stride, n=n)
            ok(lib.bfs_ptree_evaluate(tree.handle, src.ptr, m, in_stride, batch, out.ptr, out_stride, 0))
            sync()
            got = out.rows(out.contained([src.after(), tree.points.after()]))
            assert (got < np.uint64(P)).all()
            for b in range(batch):
                for i in samples:
                    assert int(got[b, i]) == horner(coeffs[b], pts[i]), (m, b, i)
        # interpolation
        in_stride = n + 2
        values = [[rng.randrange(P) for _ in range(n)] for _ in range(batch)]
        src = Input("values", strided(np.array(values, dtype=np.uint64), in_stride, np.arange(1, batch * in_stride + 1, dtype=np.uint64)))
        out = Arena(batch=batch, stride=out_stride, n=n)
        ok(lib.bfs_ptree_interpolate(tree.handle, src.ptr, in_stride, batch, out.ptr, out_stride, 0))
        got = out.rows(out.contained([src.after(), tree.points.after()]))
        assert (got < np.uint64(P)).all()
        for b in range(batch):
            poly = [int(v) for v in got[b]]
            for i in samples:
                assert horner(poly, pts[i]) == values[b][i], (b, i)


@pytest.mark.parametrize("n", [5, 64, 65, 1000])
def test_interpolation_over_two_equal_points_writes_nothing(lib, n):
    """BFS_ERR_ZERO_IN_BATCH_INVERSE, and the painted output is still all paint"""
    rng = random.Random(SEED + 7 * n)
    pts = distinct_points(rng, n)
    pts[n - 1] = pts[n // 3]
    batch, in_stride, out_stride = 3, n + 2, n + 5
    with Tree(lib, pts) as tree:
        src = Input("values", residues_plain(batch * in_stride, n))
        out = Arena(batch=batch, stride=out_stride, n=n)
        assert lib.bfs_ptree_interpolate(tree.handle, src.ptr, in_stride, batch, out.ptr, out_stride, 0) == BFS_ERR_ZERO_IN_BATCH_INVERSE
        after = out.contained([src.after(), tree.points.after()])
        assert (after == np.uint64(PAINT_WORD)).all()


def residues_plain(count, seed):
    return np.random.default_rng(SEED + seed).integers(0, P, count, dtype=np.uint64)


# ------------------------------------------------------------------------------------------------ Merkle trees
MERKLE_SIZES = [1, 2, 3, 5, 255, 257, 1000, 4097]


def node_arena(leaves):
    """2 npo2 digests of painted bytes inside guards; the result is digests 1 .. npo2 + leaves - 1: digest 0 ("head gap") and the
    slots of absent leaves ("gap 0") stay paint"""
    npo2 = cc.tree_shape(leaves)[0]
    return Arena(Layout(dtype=np.uint8, results=[(64, (npo2 + leaves - 1) * 64)], payload=2 * npo2 * 64)), npo2


def check_nodes(arena, npo2, leaves, tree, inputs):
    after = arena.contained(inputs)
    got = arena.layout.payload_of(after).tobytes()
    assert len(tree.nodes) == 2 * npo2
    wrong = [k for k in range(1, npo2 + leaves) if got[64 * k:64 * k + 64] != tree.nodes[k]]
    assert wrong == [], "%d nodes differ, first at heap index %d" % (len(wrong), wrong[0])
    assert got[:64] == bytes([PAINT_BYTE]) * 64 and got[64 * (npo2 + leaves):] == bytes([PAINT_BYTE]) * (64 * (npo2 - leaves))
    return got


@pytest.mark.parametrize("n", MERKLE_SIZES)
def test_merkle_build_xfe_and_open(lib, oracle, n):
    stride = n + 3
    soa = residues(oracle, 20 + n, 3 * n).reshape(3, n)
    if n > 5:
        soa[:, 3], soa[1:, 4], soa[2, 5] = 0, 0, 0           # zero, one and two stored coefficients: other pickle templates
    src = Input("codeword", strided(soa, stride, residues(oracle, 21, 3 * stride)))
    nodes, npo2 = node_arena(n)
    ok(lib.bfs_merkle_build_xfe(src.ptr, stride, n, nodes.ptr, 0))
    sync()
    tree, _ = oracle.xfe_merkle(soa)
    check_nodes(nodes, npo2, n, tree, [src.after()])
    if n >= 2:
        # bfs_merkle_open into a host buffer inside a painted array: leaf 0, whose siblings all exist
        depth, guard = npo2.bit_length() - 1, 256
        host = np.full(2 * guard + 64 * depth, PAINT_BYTE, dtype=np.uint8)
        ok(lib.bfs_merkle_open(nodes.ptr, depth, 0, host.ctypes.data + guard, 0))
        sync()
        path = host[guard:guard + 64 * depth].tobytes()
        assert [path[64 * k:64 * k + 64] for k in range(depth)] == tree.open(0)
        assert (host[:guard] == PAINT_BYTE).all() and (host[guard + 64 * depth:] == PAINT_BYTE).all()
        check_nodes(nodes, npo2, n, tree, [src.after()])       # opening reads


@pytest.mark.parametrize("n", MERKLE_SIZES)
def test_merkle_build_bfe(lib, oracle, n):
    values = residues(oracle, 30 + n, n)
    values[:min(n, 3)] = np.array([0, 255, P - 1], dtype=np.uint64)[:min(n, 3)]
    src = Input("values", values)
    nodes, npo2 = node_arena(n)
    ok(lib.bfs_merkle_build_bfe(src.ptr, n, nodes.ptr, 0))
    sync()
    check_nodes(nodes, npo2, n, oracle.MerkleOracle([cc.bfe_preimage(values, i) for i in range(n)]), [src.after()])


@pytest.mark.parametrize("n", MERKLE_SIZES)
def test_merkle_build_bytes(lib, oracle, n):
    """caller-pickled leaves of 0 to 299 bytes, each in whole words"""
    rng = np.random.default_rng(SEED + n)
    preimages = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, 300, n)]
    lengths = np.array([len(b) for b in preimages], dtype=np.uint32)
    words = (lengths.astype(np.uint64) + np.uint64(7)) // np.uint64(8)
    offsets = np.zeros(n, dtype=np.uint64)
    np.cumsum(words[:-1], out=offsets[1:])
    blob = rng.integers(0, 256, max(int(words.sum()), 1) * 8, dtype=np.uint8)          # junk behind every message's last byte
    for b, off in zip(preimages, offsets):
        blob[int(off) * 8:int(off) * 8 + len(b)] = np.frombuffer(b, dtype=np.uint8)
    data, offs, lens = Input("data", blob), Input("word offsets", offsets), Input("lengths", lengths.view(np.uint8))
    nodes, npo2 = node_arena(n)
    ok(lib.bfs_merkle_build_bytes(data.ptr, offs.ptr, lens.ptr, n, nodes.ptr, 0))
    sync()
    check_nodes(nodes, npo2, n, oracle.MerkleOracle(preimages), [data.after(), offs.after(), lens.after()])


@pytest.mark.parametrize("log_n", [10, 17])
@pytest.mark.parametrize("a", [2, 4, 8])
def test_merkle_build_xfe_cosets(lib, oracle, a, log_n):
    """limb_stride = n + 8; the codeword is untouched.  At 2^10 every node against hashlib over the oracle's pickles of the tuples; at
    2^17, as tests/test_gpu_fri_coset.py does for trees too large to pickle in a test's time, every parent is hashlib's hash of its
    children as written and the leaves at the workgroup edges, the last ones and 500 seeded ones are hashlib's over the oracle's
    pickle of their tuple."""
    n = 1 << log_n
    q, stride = n // a, n + 8
    cw = coset_model.tree_codeword(oracle, SEED + log_n + a, n, a, stride=stride, planted="full")
    src = Input("codeword", cw)
    nodes, npo2 = node_arena(q)
    assert npo2 == q
    ok(lib.bfs_merkle_build_xfe_cosets(src.ptr, stride, n, a.bit_length() - 1, nodes.ptr, 0))
    sync()
    if log_n == 10:
        class Want:
            nodes = coset_model.tree_nodes(oracle, cw, n, a)
        check_nodes(nodes, q, q, Want, [src.after()])
        return
    after = nodes.contained([src.after()])
    raw = nodes.layout.payload_of(after).tobytes()
    assert raw[:64] == bytes([PAINT_BYTE]) * 64
    wrong = [i for i in range(1, q) if hashlib.blake2b(raw[128 * i:128 * i + 128]).digest() != raw[64 * i:64 * i + 64]]
    assert wrong == [], "%d parents differ from blake2b of their children, first at heap index %d" % (len(wrong), wrong[0])
    rows = sorted(set(coset_model.EDGE_ROWS) | {q - 1 - r for r in coset_model.EDGE_ROWS} | {int(r) for r in np.random.RandomState(a).randint(0, q, 500)})
    for row in rows:
        tup = tuple(oracle.make_xfe([int(cw[y, row + j * q]) for y in range(3)]) for j in range(a))
        assert raw[64 * (q + row):64 * (q + row) + 64] == hashlib.blake2b(oracle.dumps(tup)).digest(), "leaf %d" % row


def test_merkle_build_rows_range(lib, oracle):
    """2^8 rows from the middle of columns of 2^10 rows (two extension and two base columns, salted): the subtree over these rows,
    columns and salts untouched"""
    from stark_brainfuck_amd import _lib
    n, total, first = 1 << 8, 1 << 10, 384
    rng = np.random.default_rng(SEED)
    columns = [residues(oracle, 40, 3 * total).reshape(3, total), residues(oracle, 41, total), residues(oracle, 42, 3 * total).reshape(3, total),
               residues(oracle, 43, total)]
    columns[2][1:, ::3] = 0
    inputs = [Input("column %d" % k, c) for k, c in enumerate(columns)]
    rc = (_lib.RowColumn * len(columns))()
    for k, (c, d) in enumerate(zip(columns, inputs)):
        rc[k].d_values, rc[k].is_ext, rc[k].field_id = d.address(first), int(c.ndim == 2), 0
    salts = rng.integers(0, 256, 24 * n, dtype=np.uint8).tobytes()
    keep = ctypes.create_string_buffer(salts, len(salts))
    nodes, npo2 = node_arena(n)
    ok(lib.bfs_merkle_build_rows_range(rc, len(columns), n, total, ctypes.cast(keep, ctypes.c_void_p), 0, nodes.ptr, 0))
    sync()
    window = [np.ascontiguousarray(c[..., first:first + n]) for c in columns]
    tree = oracle.MerkleOracle([cc.row_preimage(window, i, salts[24 * i:24 * i + 24]) for i in range(n)])
    check_nodes(nodes, npo2, n, tree, [d.after() for d in inputs])
    assert keep.raw == salts


# ------------------------------------------------------------------------------------------------ random fills
@pytest.mark.parametrize("nwords", [8, 64, 8008])
def test_random_fill(lib, nwords):
    """64-byte block j = BLAKE2b-512(seed || j); a count that is no multiple of 8 is refused and writes nothing"""
    seed = bytes(range(50, 82))
    out = Arena(batch=1, stride=nwords, n=nwords)
    ok(lib.bfs_random_fill(seed, out.ptr, nwords, 0))
    sync()
    got = out.rows(out.contained())[0].tobytes()
    assert got == b"".join(hashlib.blake2b(seed + j.to_bytes(8, "little")).digest() for j in range(nwords // 8))
    for bad in (nwords - 1, nwords + 4):
        refused = Arena(batch=1, stride=nwords + 8, n=nwords + 8)
        assert lib.bfs_random_fill(seed, refused.ptr, bad, 0) == BFS_ERR_BAD_ARG
        sync()
        assert (refused.contained() == np.uint64(PAINT_WORD)).all()


@pytest.mark.parametrize("count", [1, 2, 7, 64, 1000])
def test_xfe_sample_fill(lib, count):
    """limb_stride = count + 3; expected values from the hashlib construction of test_device_side_sampling_of_the_randomizer_polynomial:
    element i = ExtensionField.sample of bytes [27 i, 27 i + 27) of the first 63 bytes of every BLAKE2b-512(seed || block)"""
    seed = bytes(range(100, 132))
    out = Arena(batch=3, stride=count + 3, n=count)
    ok(lib.bfs_xfe_sample_fill(seed, out.ptr, count, count + 3, 0))
    sync()
    got = out.rows(out.contained())
    blocks = (27 * count + 62) // 63
    stream = b"".join(hashlib.blake2b(seed + b.to_bytes(8, "little")).digest()[:63] for b in range(blocks))
    want = np.array([[int.from_bytes(stream[27 * i + 9 * j:27 * i + 9 * j + 9], "big") % P for i in range(count)] for j in range(3)], dtype=np.uint64)
    assert (got == want).all()


# ------------------------------------------------------------------------------------------------ scans
def scan_case(rng, kind, ncols, use_mask, before, shift1, n):
    """one scan's operands and what the host primitive bfs_xfe_scan makes of them"""
    from stark_brainfuck_amd.table import Table
    cols = rng.integers(0, P, (3, n), dtype=np.uint64)
    cols[1, rng.integers(0, n, max(1, n // 7))] = 0
    mask = rng.integers(0, 4, n) != 0
    constants = [tuple(int(v) for v in rng.integers(0, P, 3, dtype=np.uint64)) for _ in range(1 + ncols)]
    initial = tuple(int(v) for v in rng.integers(0, P, 3, dtype=np.uint64))
    shift1 %= n
    host_cols = [cols[c] for c in range(ncols)]
    if shift1:
        host_cols[0] = np.roll(host_cols[0], -shift1)
    want, want_terminal = Table.scan(kind, host_cols, mask if use_mask else None, constants, initial, before)
    d_cols = [Input("x%d" % (c + 1), cols[c]) for c in range(ncols)]
    d_mask = Input("mask", np.ascontiguousarray(mask, dtype=np.uint8)) if use_mask else None
    flat = [v for c in constants for v in c] + [0] * (12 - 3 * len(constants))
    return {"kind": kind, "before": 1 if before else 0, "shift1": shift1, "n": n, "cols": d_cols, "mask": d_mask,
            "ptrs": [c.ptr for c in d_cols] + [None] * (3 - ncols), "mask_ptr": d_mask.ptr if use_mask else None,
            "constants": (u64 * 12)(*flat), "initial": (u64 * 3)(*initial), "want": want, "want_terminal": want_terminal,
            "inputs": d_cols + ([d_mask] if use_mask else [])}


@pytest.mark.parametrize("n", [1, 255, 257, 65537, 70001])
def test_scan_on_the_device(lib, n):
    """bfs_xfe_scan_device: both kinds, with and without a mask, shift1 0 and 5, out_stride = n + 5, d_terminal three words inside an
    arena; x1, x2, x3 and the mask untouched; exact against the host primitive bfs_xfe_scan.  Above 65536 rows a thread takes two."""
    rng = np.random.default_rng(SEED + n)
    for kind, ncols, use_mask, before, shift1 in [(0, 3, True, True, 0), (0, 2, False, False, 5), (1, 3, True, False, 5), (1, 1, False, True, 0)]:
        c = scan_case(rng, kind, ncols, use_mask, before, shift1, n)
        out, term = Arena(batch=3, stride=n + 5, n=n), Arena(batch=1, stride=3, n=3)
        terminal = (u64 * 3)()
        ok(lib.bfs_xfe_scan_device(kind, c["ptrs"][0], c["ptrs"][1], c["ptrs"][2], c["shift1"], c["mask_ptr"], n, c["constants"], c["initial"],
                                   c["before"], out.ptr, n + 5, term.ptr, terminal, 0))
        inputs = [i.after() for i in c["inputs"]]
        case = (kind, ncols, use_mask, before, shift1)
        assert (out.rows(out.contained(inputs)) == c["want"]).all(), case
        assert tuple(int(v) for v in term.rows(term.contained())[0]) == c["want_terminal"], case
        assert tuple(int(v) for v in terminal) == c["want_terminal"], case


def test_scans_side_by_side_in_one_arena(lib):
    """bfs_xfe_scan_device_many: four scans of 1, 300, 4099 and 70001 rows whose outputs lie next to each other in ONE arena (the
    scans need different numbers of workgroups, so those of the short ones return early), the terminals next to each other in another"""
    from stark_brainfuck_amd import _lib
    rng = np.random.default_rng(SEED + 77)
    plans = [(0, 3, True, True, 0, 1), (1, 2, False, False, 5, 300), (0, 1, True, False, 5, 4099), (1, 3, True, True, 0, 70001)]
    cases = [scan_case(rng, *plan) for plan in plans]
    results, bases, at = [], [], 0
    for c in cases:
        stride = c["n"] + 5
        bases.append(at)
        results += [(at + l * stride, c["n"]) for l in range(3)]
        at += 3 * stride
    out = Arena(Layout(results=results, payload=at))
    terms = Arena(batch=len(cases), stride=8, n=3)
    specs = [_lib.ScanSpec(c["kind"], c["before"], c["ptrs"][0], c["ptrs"][1], c["ptrs"][2], c["shift1"], c["mask_ptr"], c["n"], c["constants"],
                           c["initial"], out.address(base), c["n"] + 5, terms.address(8 * k)) for k, (c, base) in enumerate(zip(cases, bases))]
    ok(lib.bfs_xfe_scan_device_many((_lib.ScanSpec * len(specs))(*specs), len(specs), 0))
    after = out.contained([i.after() for c in cases for i in c["inputs"]])
    got_terms = terms.rows(terms.contained())
    for k, (c, plan) in enumerate(zip(cases, plans)):
        got = np.stack([out.layout.result(after, 3 * k + l) for l in range(3)])
        assert (got == c["want"]).all(), plan
        assert tuple(int(v) for v in got_terms[k]) == c["want_terminal"], plan


def test_scans_refuse_outputs_that_overlap_operands(lib):
    """the header forbids it (x1 is read shift1 rows ahead by another thread, and every operand is read twice): BFS_ERR_BAD_ARG from
    the arguments alone, nothing written -- an output plane on x1, on the tail of the mask, the device terminal on x2, and in
    bfs_xfe_scan_device_many the output of one scan on an operand of another"""
    from stark_brainfuck_amd import _lib
    rng = np.random.default_rng(SEED + 78)
    n = 300
    c = scan_case(rng, 0, 3, True, True, 5, n)
    out, term = Arena(batch=3, stride=n + 5, n=n), Arena(batch=1, stride=3, n=3)
    # operands inside arenas of their own, so that the refused calls' outputs lie inside allocations as well
    x1 = Arena(Layout(results=[], payload=3 * (n + 5)))
    x1.fill(0, rng.integers(0, P, n, dtype=np.uint64))
    mask = Arena(Layout(dtype=np.uint8, results=[], payload=8 * 3 * (n + 5)))
    mask.fill(8 * 3 * (n + 5) - n, rng.integers(0, 2, n, dtype=np.uint8))
    x2 = Arena(Layout(results=[], payload=n))
    x2.fill(0, rng.integers(0, P, n, dtype=np.uint64))

    def call(d_x1, d_x2, d_mask, d_out, d_terminal):
        return lib.bfs_xfe_scan_device(0, d_x1, d_x2, c["ptrs"][2], 5, d_mask, n, c["constants"], c["initial"], 1, d_out, n + 5, d_terminal, None, 0)
    assert call(x1.ptr, c["ptrs"][1], c["mask_ptr"], x1.ptr, term.ptr) == BFS_ERR_BAD_ARG and b"overlaps" in lib.bfs_last_error()
    assert call(c["ptrs"][0], c["ptrs"][1], mask.address(8 * 3 * (n + 5) - n), mask.ptr, term.ptr) == BFS_ERR_BAD_ARG
    assert call(c["ptrs"][0], x2.ptr, c["mask_ptr"], out.ptr, x2.address(n - 3)) == BFS_ERR_BAD_ARG
    other = scan_case(rng, 1, 1, False, False, 0, n)
    specs = [_lib.ScanSpec(0, 1, c["ptrs"][0], c["ptrs"][1], c["ptrs"][2], 5, c["mask_ptr"], n, c["constants"], c["initial"], x1.ptr, n + 5, term.ptr),
             _lib.ScanSpec(1, 0, x1.ptr, None, None, 0, None, n, other["constants"], other["initial"], out.ptr, n + 5, None)]
    assert lib.bfs_xfe_scan_device_many((_lib.ScanSpec * 2)(*specs), 2, 0) == BFS_ERR_BAD_ARG and b"scan 0 overlaps an operand of scan 1" in lib.bfs_last_error()
    sync()
    for arena in (out, term, x1, mask, x2):
        arena.contained([i.after() for i in c["inputs"]])
    assert (out.snapshot() == np.uint64(PAINT_WORD)).all()
    # and the same operands with outputs of their own are served
    ok(call(x1.ptr, x2.ptr, mask.address(8 * 3 * (n + 5) - n), out.ptr, term.ptr))
    sync()
    for arena in (x1, mask, x2):
        arena.contained()


# ------------------------------------------------------------------------------------------------ trace padding
def test_trace_pad_five_tables_in_one_call(lib):
    """heights 4096, 512, 256, 1 and 2 with 2500, 512 (= the height), 100, 0 and 1 rows; every output and every mask -- the ones a
    table's kind does not use as well -- in an arena of its own; the rows are untouched"""
    from stark_brainfuck_amd import _lib
    rng = np.random.default_rng(SEED + 5)
    heights, counts = [4096, 512, 256, 1, 2], [2500, 512, 100, 0, 1]
    edge = np.array([0, 1, 44, 46, P - 1, P, P + 5, (1 << 64) - 1], dtype=np.uint64)
    tables, raws, outs, masks, structs = [], [], [], [], (_lib.TracePadTable * 5)()
    for t, (h, k) in enumerate(zip(heights, counts)):
        stride = PAD_WIDTH[t] + 2
        rows = rng.integers(0, 1 << 63, (k, stride), dtype=np.uint64)
        rows = np.where(rng.integers(0, 3, (k, stride)) == 0, edge[rng.integers(0, len(edge), (k, stride))], rows)
        if t == 1:
            rows[:, 0] = np.sort(rng.integers(0, k // 3, k).astype(np.uint64))          # repeated addresses, as in a real table
        tables.append(rows)
        raws.append(Input("rows of table %d" % t, rows) if k else None)
        outs.append(Arena(batch=1, stride=PAD_WIDTH[t] * h, n=PAD_WIDTH[t] * h))
        masks.append([Arena(Layout(dtype=np.uint8, results=[(0, h)] if m < PAD_MASKS[t] else [], payload=h)) for m in range(3)])
        s = structs[t]
        s.d_rows, s.rows, s.row_stride, s.height = (raws[t].ptr if k else None), k, (stride if k else 0), h
        s.d_out, s.d_mask0, s.d_mask1, s.d_mask2, s.kind, s.width = outs[t].ptr, masks[t][0].ptr, masks[t][1].ptr, masks[t][2].ptr, t, PAD_WIDTH[t]
    ok(lib.bfs_trace_pad(structs, 5, 0))
    sync()
    for t, (h, rows) in enumerate(zip(heights, tables)):
        want, want_masks = padded(t, rows, PAD_WIDTH[t], h)
        after = outs[t].contained([raws[t].after()] if raws[t] else [])
        assert outs[t].rows(after)[0].reshape(PAD_WIDTH[t], h).tolist() == want, "table %d" % t
        for m in range(3):
            got = masks[t][m].contained()
            if m < PAD_MASKS[t]:
                assert masks[t][m].layout.result(got).tolist() == want_masks[m], "table %d mask %d" % (t, m)
            else:
                assert (got == PAINT_BYTE).all(), "table %d has no mask %d" % (t, m)


# ------------------------------------------------------------------------------------------------ FRI folds
@functools.lru_cache(maxsize=None)
def fold_codeword(log_n):
    """(3, 2^log_n) residues, shared by the fold tests and never changed"""
    from oracle import ref_oracle as o
    cw = o.felt_array(SEED + 900 + log_n, 0, 3 << log_n).reshape(3, 1 << log_n)
    cw.setflags(write=False)
    return cw


def fold_check(oracle, cw, got, log_n, k, alpha, omega):
    """got: (3, n >> k).  Up to 2^16 every element against oracle.fri_fold applied k times (tests/fri_folding_model.py); above, where
    that takes many seconds, the elements at the edges of the kernel's grid (4096 workgroups of 256) and 4096 seeded ones: element c
    is the k-fold of the a = 2^k inputs c + j n / a, a codeword of its own over the coset offset * omega^c * <omega^(n / a)>."""
    n, a = 1 << log_n, 1 << k
    q = n >> k
    assert got.shape == (3, q) and (got < np.uint64(P)).all()
    if log_n <= 16:
        want, _, _ = folding_model.fold_round(oracle, cw, alpha, OFFSET, omega, k)
        assert (got == want).all()
        return
    rng = random.Random(log_n + k)
    grid = 4096 * 256
    picks = sorted({c for c in (0, 1, 255, 256, grid - 1, grid, grid + 1, 2 * grid - 1, 2 * grid, q - 1) if c < q} | {rng.randrange(q) for _ in range(4096)})
    step = oracle.power(omega, q)
    for c in picks:
        sub = np.ascontiguousarray(cw[:, c::q])
        assert sub.shape == (3, a)
        want, _, _ = folding_model.fold_round(oracle, sub, alpha, oracle.mul(OFFSET, oracle.power(omega, c)), step, k)
        assert (got[:, 0 if q == 1 else c] == want[:, 0]).all(), c


def fold_call(lib, k, single, d_in, in_stride, d_out, out_stride, log_n, alpha, omega):
    if single:
        return lib.bfs_xfe_fold(d_in, in_stride, d_out, out_stride, log_n, (u64 * 3)(*alpha), OFFSET, omega, 0)
    return lib.bfs_xfe_fold_multi(d_in, in_stride, d_out, out_stride, log_n, k, (u64 * 3)(*alpha), OFFSET, omega, 0)


@pytest.mark.parametrize("size", ["smallest", "2^10", "2^23"])
@pytest.mark.parametrize("entry,k", [("bfs_xfe_fold", 1), ("bfs_xfe_fold_multi", 2), ("bfs_xfe_fold_multi", 3)])
def test_fold_out_of_place_and_in_place(lib, oracle, entry, k, size):
    """log_n = k is the smallest codeword; at 2^23 the output has more than 4096 * 256 elements for every k, so the grid-stride loop
    runs.  Out of place with out_stride = out_len + 9 and the input untouched; in place (d_out == d_in, equal strides): thread i
    reads in[i] itself and every other read lies at or above n / 2, so the folded codeword replaces the first n / 2^k elements of each
    limb plane and the rest of the plane stays as it was."""
    log_n = {"smallest": k, "2^10": 10, "2^23": 23}[size]
    n = 1 << log_n
    q = n >> k
    cw = fold_codeword(log_n)
    alpha = [int(v) for v in residues(oracle, 950 + k, 3)]
    omega = oracle.primitive_nth_root(n)
    single = entry == "bfs_xfe_fold"
    src = Input("codeword", cw)
    out = Arena(batch=3, stride=q + 9, n=q)
    ok(fold_call(lib, k, single, src.ptr, n, out.ptr, q + 9, log_n, alpha, omega))
    sync()
    apart = out.rows(out.contained([src.after()]))
    fold_check(oracle, cw, apart, log_n, k, alpha, omega)
    arena = Arena(Layout(results=[(l * n, q) for l in range(3)], payload=3 * n))
    arena.fill(0, cw)
    ok(fold_call(lib, k, single, arena.ptr, n, arena.ptr, n, log_n, alpha, omega))
    sync()
    after = arena.contained()
    assert (np.stack([arena.layout.result(after, l) for l in range(3)]) == apart).all(), "in place"


# ------------------------------------------------------------------------------------------------ Fri.prove
@pytest.mark.parametrize("log_n", [10, 17])
@pytest.mark.parametrize("coset_leaves", [False, True])
@pytest.mark.parametrize("a", [2, 4, 8])
def test_fri_prove_leaves_the_callers_codeword_and_tree_alone(sb, oracle, a, coset_leaves, log_n):
    """Fri.prove hands the caller's codeword to the fused tree and fold kernels (and, with coset leaves, to coset_leaves_kernel) through
    non-const pointers: the codeword, inside an arena whose limb planes are longer than the codeword, is bit-identical afterwards and
    so is everything around it; the same for the nodes of a round0_tree handed in.  The proof verifies; that these proofs are the
    protocol models' byte for byte is tests/test_gpu_fri_folding.py's and tests/test_gpu_fri_coset.py's subject."""
    N, expansion, t = 1 << log_n, 4, 4
    omega = oracle.primitive_nth_root(N)
    cw = folding_model.codeword_of(oracle, SEED + N, N, expansion, OFFSET, omega)
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    assert BF.generator().value == OFFSET
    fri = sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, expansion, t, XF, folding_factor=a, coset_leaves=coset_leaves)
    stride = N + 11
    arena = Arena(batch=3, stride=stride, n=N)
    arena.fill_rows(cw)

    from stark_brainfuck_amd.device import DeviceView
    codeword = sb.XArray(DeviceView(arena.buf, arena.layout.guard, 3 * stride), N, stride=stride)
    roots = []
    for with_tree in (False, True):
        tree = None
        if with_tree:
            tree = sb.CosetMerkle(codeword, a) if coset_leaves else sb.Merkle(codeword)
            sync()
            nodes_before = tree._nodes.to_numpy()
        ps = sb.ProofStream()
        indices = fri.prove(codeword, ps, round0_tree=tree)
        sync()
        after = arena.snapshot()
        assert np.array_equal(after, arena.image), "the caller's codeword or its surroundings changed (with_tree=%s)" % with_tree
        if with_tree:
            assert np.array_equal(tree._nodes.to_numpy(), nodes_before), "the round0_tree handed in changed"
            root = tree.root()
        else:
            root = (sb.CosetMerkle(codeword, a) if coset_leaves else sb.Merkle(codeword)).root()
        assert len(indices) == t
        assert fri.verify(sb.ProofStream().deserialize(ps.serialize()), root) is True
        roots.append((root, ps.serialize()))
    assert roots[0] == roots[1], "the proof with a round0_tree differs from the proof without"


# ------------------------------------------------------------------------------------------------ row-range entry points
# (first row, number of rows) at 2^12: everything, the first row, the last row, an odd piece, and from one row before the middle
# both the three rows 2047 .. 2049 and everything up to the end.  (2047, 2050) itself would end one row past the domain: refused.
ROW_WINDOWS = [(0, 1 << 12), (0, 1), ((1 << 12) - 1, 1), (17, 255), (2047, 3), (2047, 2049)]
ROW_WINDOW_PAST_THE_END = (2047, 2050)


def test_zerofier_inverses_by_row_windows(lib, oracle):
    """bfs_zerofier_inverses_rows at 2^12 into a painted FULL buffer of three codewords: rows outside the window stay paint, rows
    inside equal the full-range call, which is the oracle's inverse of x - 1, x - omicron^-1 and x^256 - 1 at every point"""
    log_n = 12
    n = 1 << log_n
    omega = oracle.primitive_nth_root(n)
    omicron_inv = oracle.inv(oracle.primitive_nth_root(256))
    is_power, values = (ctypes.c_uint32 * 3)(0, 0, 1), (u64 * 3)(1, omicron_inv, 8)
    x = oracle.scale(omega, np.full(n, OFFSET, dtype=np.uint64))                      # offset * omega^i
    x256 = x.copy()
    for _ in range(8):
        x256 = oracle.hadamard(x256, x256)
    sub = lambda v, c: np.array([(int(e) - c) % P for e in v], dtype=np.uint64)
    want = np.stack([oracle.batch_inverse(sub(x, 1)), oracle.batch_inverse(sub(x, omicron_inv)), oracle.batch_inverse(sub(x256, 1))])
    for first, count in ROW_WINDOWS:
        arena = Arena(Layout(results=[(k * n + first, count) for k in range(3)], payload=3 * n))
        ok(lib.bfs_zerofier_inverses_rows(log_n, OFFSET, omega, 3, is_power, values, arena.ptr, first, count, 0))
        sync()
        after = arena.contained()
        got = np.stack([arena.layout.result(after, k) for k in range(3)])
        assert (got == want[:, first:first + count]).all(), (first, count)
    full = Arena(batch=3, stride=n, n=n)
    ok(lib.bfs_zerofier_inverses(log_n, OFFSET, omega, 3, is_power, values, full.ptr, 0))
    sync()
    assert (full.rows(full.contained()) == want).all()
    refused = Arena(Layout(results=[], payload=3 * n))
    assert lib.bfs_zerofier_inverses_rows(log_n, OFFSET, omega, 3, is_power, values, refused.ptr, *ROW_WINDOW_PAST_THE_END, 0) == BFS_ERR_BAD_ARG
    sync()
    refused.contained()


def test_difference_combine_by_row_windows(lib, oracle):
    """bfs_difference_combine_rows at 2^12 on an accumulator of seeded residues: rows outside the window unchanged, rows inside equal
    the full-range call, which is acc + (wa + wb x^shift) (lhs - rhs) / (x - 1) in the oracle's extension arithmetic; with the
    codeword of 1 / (x - 1) handed in and computed on the spot; lhs, rhs and the inverses untouched"""
    from stark_brainfuck_amd import _lib
    log_n = 12
    n = 1 << log_n
    omega = oracle.primitive_nth_root(n)
    lhs, rhs, acc = (residues(oracle, 60 + k, 3 * n).reshape(3, n) for k in range(3))
    weight = _lib.CombWeight()
    wa, wb, shift = [int(v) for v in residues(oracle, 63, 3)], [int(v) for v in residues(oracle, 64, 3)], 1000
    weight.wa, weight.wb, weight.shift = (u64 * 3)(*wa), (u64 * 3)(*wb), shift
    x = oracle.scale(omega, np.full(n, OFFSET, dtype=np.uint64))
    inv = oracle.batch_inverse(np.array([(int(e) - 1) % P for e in x], dtype=np.uint64))
    want = np.empty((3, n), dtype=np.uint64)
    for i in range(n):
        xs = oracle.power(int(x[i]), shift)
        w = oracle.xadd(wa, [oracle.mul(v, xs) for v in wb])
        q = [oracle.mul(oracle.sub(int(lhs[l, i]), int(rhs[l, i])), int(inv[i])) for l in range(3)]
        want[:, i] = oracle.xadd([int(v) for v in acc[:, i]], oracle.xmul(w, q))
    d_lhs, d_rhs, d_inv = Input("lhs", lhs), Input("rhs", rhs), Input("1 / (x - 1)", inv)
    for given in (True, False):
        inputs = [d_lhs, d_rhs] + ([d_inv] if given else [])
        full = Arena(batch=3, stride=n, n=n)
        full.fill_rows(acc)
        ok(lib.bfs_difference_combine(d_lhs.ptr, d_rhs.ptr, log_n, OFFSET, omega, ctypes.byref(weight), full.ptr, d_inv.ptr if given else None, 0))
        sync()
        assert (full.rows(full.contained([i.after() for i in inputs])) == want).all(), given
        for first, count in ROW_WINDOWS:
            arena = Arena(Layout(results=[(l * n + first, count) for l in range(3)], payload=3 * n))
            arena.fill(0, acc)
            ok(lib.bfs_difference_combine_rows(d_lhs.ptr, d_rhs.ptr, log_n, OFFSET, omega, ctypes.byref(weight), arena.ptr,
                                               d_inv.ptr if given else None, first, count, 0))
            sync()
            after = arena.contained([i.after() for i in inputs])
            got = np.stack([arena.layout.result(after, l) for l in range(3)])
            assert (got == want[:, first:first + count]).all(), (given, first, count)
        refused = Arena(Layout(results=[], payload=3 * n))
        refused.fill(0, acc)
        assert lib.bfs_difference_combine_rows(d_lhs.ptr, d_rhs.ptr, log_n, OFFSET, omega, ctypes.byref(weight), refused.ptr,
                                               d_inv.ptr if given else None, *ROW_WINDOW_PAST_THE_END, 0) == BFS_ERR_BAD_ARG
        sync()
        refused.contained()


def test_trace_pad_refuses_outputs_that_overlap_rows(lib):
    """the header forbids it (the call transposes): BFS_ERR_BAD_ARG and nothing written when a table's output or a mask lies on its
    own rows or on another table's"""
    from stark_brainfuck_amd import _lib
    rng = np.random.default_rng(SEED + 6)
    h = 64
    rows = Arena(Layout(results=[], payload=9 * h))
    rows.fill(0, rng.integers(0, P, 9 * h, dtype=np.uint64))
    io_rows = Input("input rows", rng.integers(0, P, h, dtype=np.uint64))
    out, io_out = Arena(batch=1, stride=7 * h, n=7 * h), Arena(batch=1, stride=h, n=h)
    masks = [Arena(Layout(dtype=np.uint8, results=[(0, h)], payload=h)) for _ in range(3)]

    def call(d_out0, d_mask2, d_out1):
        t = (_lib.TracePadTable * 2)()
        t[0].d_rows, t[0].rows, t[0].row_stride, t[0].height, t[0].kind, t[0].width = rows.ptr, h, 9, h, 0, 7
        t[0].d_out, t[0].d_mask0, t[0].d_mask1, t[0].d_mask2 = d_out0, masks[0].ptr, masks[1].ptr, d_mask2
        t[1].d_rows, t[1].rows, t[1].row_stride, t[1].height, t[1].kind, t[1].width, t[1].d_out = io_rows.ptr, h, 1, h, 3, 1, d_out1
        return lib.bfs_trace_pad(t, 2, 0)
    assert call(rows.ptr, masks[2].ptr, io_out.ptr) == BFS_ERR_BAD_ARG and b"overlaps" in lib.bfs_last_error()
    assert call(out.ptr, rows.address(9 * h - 8), io_out.ptr) == BFS_ERR_BAD_ARG          # a mask on the last row
    assert call(out.ptr, masks[2].ptr, rows.address(h)) == BFS_ERR_BAD_ARG                # the input table's output on the processor's rows
    sync()
    for arena in [rows, out, io_out] + masks:
        after = arena.contained([io_rows.after()])
    assert (out.snapshot() == np.uint64(PAINT_WORD)).all() and (io_out.snapshot() == np.uint64(PAINT_WORD)).all()
    ok(call(out.ptr, masks[2].ptr, io_out.ptr))
    sync()
    rows.contained([io_rows.after()])
    want, _ = padded(0, rows.layout.payload_of(rows.image).reshape(h, 9), 7, h)
    assert out.rows(out.contained())[0].reshape(7, h).tolist() == want
