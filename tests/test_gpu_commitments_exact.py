"""The commitment layer checked exactly from 2^17 to 2^24 leaves.  Everything the prover says is said through a Merkle root; above
the sizes of the reference's own runs (2^16 rows, N = 2^20 for FRI) nothing compared a root, a node or a leaf digest with an
independent computation.  tests/commitment_check.py recomputes, with hashlib and CPython's pickle only:
  * every parent of every tree looked at (all sizes, ragged levels included);
  * leaf digests from host copies of the committed data: all of them up to 2^18 leaves, above that on sample_rows (both ends, the
    quarters, every 2^20 / 2^16 multiple, the powers of two, 4096 uniform rows) plus the rows interesting_rows finds or a case plants;
  * the FRI transcript from the checked trees, against the bytes Fri.prove writes.
(a) the prover's base, extension and combination trees for the six programs of test_gpu_prover_pointwise (2^17 ... 2^24), from the
fixed stream and once with device-made salts; (b) Fri.commit / Fri.prove at N = 2^22 and 2^24 round by round; (c) synthetic trees
through the four C ABI builders at ragged sizes and with planted leaf classes; (d) the two implementations of the row leaves
against each other over every leaf, in child processes.  Each case prints what it measured (run with -s to see it)."""
import ctypes
import gc
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

import commitment_check as cc
from conftest import ROOT
from oracle import ref_oracle as oracle
from test_gpu_prover_pointwise import PROGRAMS, _prove

pytestmark = pytest.mark.gpu
P = oracle.P
ALL_LEAVES_MAX = 1 << 18          # trees of at most this many leaves: every leaf digest is recomputed
ROW_GROUP, ELEMENT_GROUP = 256, 64      # LEAF_THREADS of the row-leaf kernels and of the element-leaf kernels


def _lib_and_device():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from stark_brainfuck_amd import _lib, device
    return _lib, _lib.load(), device


def _note(*args):
    print("[commitments]", *args, flush=True)


def _tree_failures(nodes, n, rows, preimage_of, label):
    """all parents and the leaves `rows` of the heap in the device buffer `nodes` (anything with to_numpy(count, offset) in words)"""
    npo2, depth = cc.tree_shape(n)
    started = time.time()
    failures = cc.check_parents(cc.heap_reader(nodes.to_numpy), depth, n)
    parents_seconds = time.time() - started
    started = time.time()
    leaves = nodes.to_numpy(8 * n, offset=8 * npo2)
    rows = list(rows)
    failures += cc.check_leaves(cc.digest_reader(leaves), rows, preimage_of)
    _note("%s: %d leaves, %d parents in %.1f s, %d leaf digests in %.1f s, %d failures"
          % (label, n, npo2 - 1, parents_seconds, len(rows), time.time() - started, len(failures)))
    return [(kind, label + ": " + message) for kind, message in failures]


def _assert_none(failures):
    assert not failures, "\n".join("%s: %s" % f for f in failures[:40])


def _rows_for(n, group, seed, extra=()):
    return range(n) if n <= ALL_LEAVES_MAX else cc.sample_rows(n, group, seed, extra)


# ------------------------------------------------------------------------------------------------ (a) the prover's three trees
def _salts_of(tree, n):
    if getattr(tree, "_salt_host", None) is not None:
        return tree._salt_host.raw[:24 * n]
    return tree._salts.to_numpy(3 * n).tobytes()


def _check_prover_trees(stark, proof, label):
    """the three trees of the proof `stark` has just written (keep_intermediates); returns the extension tree's row patterns"""
    last, n = stark._last, stark.fri.domain.length
    failures = []

    def base_columns():          # in the order prove() zips them: the randomizer, then every table's base columns
        yield last["randomizer_codeword"].to_numpy()
        for t in stark.tables:
            for c in range(t.base_width):
                yield t.base_codewords.to_numpy(n, offset=c * n)

    def ext_columns():
        for t in stark.tables:
            for c in range(t.full_width - t.base_width):
                yield t.ext_codewords.to_numpy(3 * n, offset=3 * c * n).reshape(3, n)

    patterns = None
    for name, columns, tree in (("base", base_columns, last["base_tree"]), ("extension", ext_columns, last["extension_tree"])):
        found, code = {}, np.zeros(n, dtype=np.int64)
        for k, column in enumerate(columns()):
            assert (column < np.uint64(P)).all(), "%s column %d holds a word >= p" % (name, k)
            found.update(cc.interesting_rows([column], [], first=k) if column.ndim == 2 else cc.interesting_rows([], [column], first=k))
            if column.ndim == 2:
                code = code * 4 + cc.stored_coefficients(column)
        rows = _rows_for(n, ROW_GROUP, n, cc.rows_of(found))
        picked = cc.PickedRows(rows)
        for column in columns():
            picked.pick(column)
        salts = _salts_of(tree, n)
        assert len(salts) == 24 * n
        failures += _tree_failures(tree._nodes, n, rows, lambda i: picked.preimage(i, salts[24 * i:24 * i + 24]), "%s %s tree" % (label, name))
        codes, counts = np.unique(code, return_counts=True)
        _note("%s %s tree: classes found / checked %s; row patterns (code: rows) %s"
              % (label, name, cc.class_counts(found), dict(zip(codes.tolist(), counts.tolist()))))
        if name == "extension":
            patterns = set(codes.tolist())
        del picked, salts, code
    combination = last["combination"].to_numpy()
    found = cc.interesting_rows([combination], [])
    rows = _rows_for(n, ELEMENT_GROUP, n + 1, cc.rows_of(found))
    failures += _tree_failures(last["combination_tree"]._nodes, n, rows, lambda i: cc.xfe_preimage(combination, i), label + " combination tree")
    _note("%s combination tree: classes found / checked %s" % (label, cc.class_counts(found)))
    _assert_none(failures)
    # the three roots are the first three 64-byte objects of the proof stream, in order, and the proof is accepted
    stream_roots = [o for o in pickle.loads(proof) if isinstance(o, bytes) and len(o) == 64][:3]
    tree_roots = [last[key]._nodes.to_numpy(8, offset=8).tobytes() for key in ("base_tree", "extension_tree", "combination_tree")]
    assert stream_roots == tree_roots
    assert [last[key].root() for key in ("base_tree", "extension_tree", "combination_tree")] == tree_roots
    assert stark.verify(proof) is True
    return patterns


def _extension_patterns(stark):
    """the row patterns (2 bits per column: stored coefficients) of the extension rows of the proof `stark` has just written"""
    n, code = stark.fri.domain.length, 0
    for t in stark.tables:
        for c in range(t.full_width - t.base_width):
            code = code * 4 + cc.stored_coefficients(t.ext_codewords.to_numpy(3 * n, offset=3 * c * n).reshape(3, n)).astype(np.int64)
    return set(np.unique(code).tolist())


@pytest.fixture(scope="module")
def seen_patterns():
    """program -> the row patterns of its extension tree: filled by the cases that prove a program anyway, completed by the test
    that asserts on it, so that its verdict is over all six programs whichever tests were selected and in whatever order"""
    return {}


@pytest.mark.parametrize("name", list(PROGRAMS))
def test_prover_trees_exact(name, monkeypatch, seen_patterns):
    stark, proof = _prove(monkeypatch, name, keep_intermediates=True)
    seen_patterns[name] = _check_prover_trees(stark, proof, name)
    assert seen_patterns[name] == _extension_patterns(stark)
    del stark
    gc.collect()
    # keep_intermediates takes the Python stage driver; the default prover (native stage driver, extension rows hashed on a library
    # thread) must write the same bytes from the same stream: the same three roots, hence the same leaves
    assert _prove(monkeypatch, name)[1] == proof, "native stage driver"
    gc.collect()


def test_prover_trees_exact_with_salts_made_on_the_device():
    """2^20, the operating system's randomness: the salts come from bfs_random_fill and are read back from the trees"""
    from stark_brainfuck_amd import salted_merkle
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    from stark_brainfuck_amd.vm import VirtualMachine
    assert salted_merkle.urandom is os.urandom
    code, inputs, log_n = PROGRAMS["nested32"]
    program = VirtualMachine.compile(code)
    running_time, input_symbols, output_symbols = VirtualMachine.run(program, input_data=list(inputs))
    matrices = VirtualMachine.simulate(program, input_data=list(input_symbols))
    stark = BrainfuckStark(running_time, len(matrices[1]), program, input_symbols, output_symbols)
    assert stark.fri.domain.length == 1 << log_n
    stark.keep_intermediates = True
    proof = stark.prove(program, *matrices)
    for key in ("base_tree", "extension_tree"):
        tree = stark._last[key]
        assert getattr(tree, "_salt_host", None) is None and tree._salts is not None
        salts = _salts_of(tree, 1 << log_n)
        assert len({salts[24 * i:24 * i + 24] for i in range(0, 1 << log_n, 997)}) == len(range(0, 1 << log_n, 997))
    _check_prover_trees(stark, proof, "nested32 (device salts)")
    del stark
    gc.collect()


def test_extension_rows_come_in_more_than_one_pattern(monkeypatch, seen_patterns):
    """hello_world reads no input, so its input-evaluation column is the zero polynomial; echo reads and writes ("nine
    row patterns"): over the six programs the extension tree is seen with at least two different row patterns.  A program no
    earlier case of this run has proven is proven here (the patterns only: a scan of its extension codewords)."""
    for name in PROGRAMS:
        if name not in seen_patterns:
            stark, _ = _prove(monkeypatch, name, keep_intermediates=True)
            seen_patterns[name] = _extension_patterns(stark)
            del stark
            gc.collect()
    _note("extension row patterns per program:", {k: sorted(v) for k, v in seen_patterns.items()})
    assert set(seen_patterns) == set(PROGRAMS)
    assert len(set().union(*seen_patterns.values())) >= 2, seen_patterns


# ------------------------------------------------------------------------------------------------ (b) FRI round by round
@pytest.mark.parametrize("log_n", [22, 24])
def test_fri_rounds_exact(log_n):
    import stark_brainfuck_amd as sb
    _lib_and_device()
    N, expansion, t = 1 << log_n, 4, 4
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    omega = oracle.primitive_nth_root(N)
    fri = sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, expansion, t, XF)
    assert (fri.domain.offset.value, fri.domain.omega.value) == (oracle.GENERATOR, omega)
    coeffs = oracle.felt_array(0xF71 + log_n, 0, 3 * (N // expansion)).reshape(3, -1)
    cw = fri.domain.xevaluate(sb.XArray.from_numpy(coeffs), as_array=True)
    ps = sb.ProofStream()
    codewords, trees = fri.commit(cw, ps)
    R = fri.num_rounds()
    lengths = [len(c) for c in codewords]
    assert lengths == [N >> r for r in range(R)] and len(trees) == R - 1
    host = [c.array.to_numpy() for c in codewords]
    assert all((h < np.uint64(P)).all() for h in host)
    failures = []
    # every tree: all parents, leaves sampled (all of them up to 2^18 elements); the stand-alone leaf kernel over every leaf
    for r, tree in enumerate(trees):
        n = lengths[r]
        found = cc.interesting_rows([host[r]], [])
        rows = _rows_for(n, ELEMENT_GROUP, n, cc.rows_of(found))
        failures += _tree_failures(tree._nodes, n, rows, lambda i, r=r: cc.xfe_preimage(host[r], i), "FRI 2^%d round %d" % (log_n, r))
        alone = sb.Merkle(codewords[r].array)
        assert alone.root() == tree.root(), "round %d: stand-alone tree" % r
        assert np.array_equal(alone._nodes.to_numpy(8 * n, offset=8 * n), tree._nodes.to_numpy(8 * n, offset=8 * n)), "round %d: leaf level" % r
        del alone
    _assert_none(failures)
    # the transcript the checked trees and the host copies of the codewords give
    out = cc.fri_transcript_from_trees(lengths, lambda r, i: host[r][:, i],
                                       lambda r, k: trees[r]._nodes.to_numpy(8, offset=8 * k).tobytes(), expansion, t)
    assert out["roots"][:-1] == [tree.root() for tree in trees]
    assert [bytes(o) for o in ps.objects[:R - 1]] == out["roots"][1:]
    # round r + 1's codeword is the fold of round r's, over the whole length, with the transcript's alpha
    w, g = omega, oracle.GENERATOR
    for r, alpha in enumerate(out["alphas"]):
        started = time.time()
        assert np.array_equal(oracle.fri_fold(host[r], alpha, g, w), host[r + 1]), "fold of round %d" % r
        if r < 3:
            _note("FRI 2^%d fold %d -> %d: %.1f s" % (log_n, r, r + 1, time.time() - started))
        w, g = oracle.mul(w, w), oracle.mul(g, g)
    root0 = trees[0].root()
    del codewords, trees
    gc.collect()
    # Fri.prove on the same codeword writes exactly those bytes
    ps2 = sb.ProofStream()
    assert fri.prove(cw, ps2) == out["indices"]
    assert ps2.serialize() == out["proof_stream"].serialize()
    vs = sb.ProofStream()
    vs.objects = list(ps2.objects)
    assert fri.verify(vs, root0)


# ------------------------------------------------------------------------------------------------ (c) synthetic trees
RAGGED = [300, 5000, 8193, 16385, 65537, 100003, (1 << 17) + 1, (1 << 18) - 1, 3 * (1 << 18) + 5, (1 << 20) + 1]
FOUR_SIZES = [300, 16385, 100003, 3 * (1 << 18) + 5]
EDGES = [0, 1, 255, 256, 65535, 65536, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 39) - 1, 1 << 39, (1 << 47) - 1, 1 << 47,
         (1 << 55) - 1, 1 << 55, (1 << 63) - 1, 1 << 63, P - 1]


def _nodes_for(n):
    from stark_brainfuck_amd.device import DeviceBuffer
    return DeviceBuffer(2 * cc.tree_shape(n)[0] * 8)


def _plant_elements(soa, rows):
    """zero elements, lifted base elements, two-coefficient elements and edge integers at `rows`, class by class in turn"""
    for j, i in enumerate(rows):
        kind = j % 4
        if kind == 0:
            soa[:, i] = 0
        elif kind == 1:
            soa[1:, i] = 0
        elif kind == 2:
            soa[2, i] = 0
        else:
            for k in range(3):
                soa[k, i] = np.uint64(EDGES[(j + k) % len(EDGES)] or (1 if k == 2 else 0))


def _plant_places(n):
    return sorted({i for i in (0, 1, 2, 3, 62, 63, 64, 65, 66, 67, n // 2, n // 2 + 1, n // 2 + 2, n // 2 + 3, n - 8, n - 7, n - 6, n - 5, n - 4, n - 3,
                               n - 2, n - 1) if 0 <= i < n})


@pytest.mark.parametrize("n", RAGGED)
def test_ragged_trees_of_extension_elements(n):
    """bfs_merkle_build_xfe just over, just under and between powers of two: the ragged level goes to the top, quad or throughput
    parents kernel by its size, and the complete level above it starts a subtree launch or not"""
    import stark_brainfuck_amd as sb
    _lib, lib, device = _lib_and_device()
    soa = oracle.felt_array(0xA000 + n, 0, 3 * n).reshape(3, n)
    planted = _plant_places(n)
    _plant_elements(soa, planted)
    arr = sb.XArray.from_numpy(soa)
    nodes = _nodes_for(n)
    _lib.check(lib.bfs_merkle_build_xfe(arr.ptr, arr.stride, n, nodes.ptr, 0))
    device.synchronize(0)
    rows = _rows_for(n, ELEMENT_GROUP, n, planted)
    _assert_none(_tree_failures(nodes, n, rows, lambda i: cc.xfe_preimage(soa, i), "xfe %d" % n))


@pytest.mark.parametrize("n", FOUR_SIZES)
def test_ragged_trees_of_base_elements(n):
    import stark_brainfuck_amd as sb
    _lib, lib, device = _lib_and_device()
    values = oracle.felt_array(0xB000 + n, 0, n)
    planted = _plant_places(n)
    for j, i in enumerate(planted):
        values[i] = np.uint64(EDGES[j % len(EDGES)])
    arr = sb.BaseArray.from_numpy(values)
    nodes = _nodes_for(n)
    _lib.check(lib.bfs_merkle_build_bfe(arr.ptr, n, nodes.ptr, 0))
    device.synchronize(0)
    _assert_none(_tree_failures(nodes, n, _rows_for(n, ELEMENT_GROUP, n, planted), lambda i: cc.bfe_preimage(values, i), "bfe %d" % n))


@pytest.mark.parametrize("n", FOUR_SIZES)
def test_ragged_trees_of_byte_strings(n):
    """bfs_merkle_build_bytes (blake2b_batch_kernel) on messages of 0 ... 400 bytes, the block-boundary lengths among them; the words
    between two messages hold random bytes that belong to no message"""
    _lib, lib, device = _lib_and_device()
    from stark_brainfuck_amd.device import DeviceBuffer
    rng = np.random.default_rng(n)
    lengths = rng.integers(0, 401, n, dtype=np.uint32)
    special = [0, 127, 128, 129, 255, 256, 257, 1, 63, 64, 65, 383, 384, 385, 400]
    planted = _plant_places(n)
    for j, i in enumerate(planted):
        lengths[i] = special[j % len(special)]
    assert set(special) <= set(lengths.tolist())
    words = (lengths.astype(np.uint64) + np.uint64(7)) // np.uint64(8)
    offsets = np.zeros(n, dtype=np.uint64)
    np.cumsum(words[:-1], out=offsets[1:])
    total = int(words.sum())
    blob = rng.integers(0, 1 << 63, total + 1, dtype=np.uint64)
    data = blob.tobytes()
    d_data, d_off = DeviceBuffer.from_numpy(blob), DeviceBuffer.from_numpy(offsets)
    d_len = DeviceBuffer.from_numpy(np.frombuffer(np.concatenate([lengths, np.zeros(n % 2, np.uint32)]).tobytes(), dtype=np.uint64))
    nodes = _nodes_for(n)
    _lib.check(lib.bfs_merkle_build_bytes(d_data.ptr, d_off.ptr, d_len.ptr, n, nodes.ptr, 0))
    device.synchronize(0)
    rows = range(n)                          # a message is there already: every leaf, at every size
    _assert_none(_tree_failures(nodes, n, rows, lambda i: data[8 * int(offsets[i]):8 * int(offsets[i]) + int(lengths[i])], "bytes %d" % n))


def _row_columns(_lib, arrays, offset=0, stride=None):
    """device copies of the columns and the bfs_row_column array over them (from row `offset` on)"""
    from stark_brainfuck_amd.device import DeviceBuffer
    bufs = [DeviceBuffer.from_numpy(np.ascontiguousarray(a).reshape(-1)) for a in arrays]
    rc = (_lib.RowColumn * len(bufs))()
    for k, (a, b) in enumerate(zip(arrays, bufs)):
        rc[k].d_values, rc[k].is_ext, rc[k].field_id = b.ptr + 8 * offset, int(a.ndim == 2), 0
    return bufs, rc


def _mixed_columns(n, seed):
    """3 extension + 5 base columns interleaved, as test_zipped_rows_commitment_on_device_vs_oracle orders them: limb planes with
    different zero patterns (0 ... 3 stored coefficients) and integers of every width among uniform ones"""
    rng = np.random.default_rng(seed)

    def column(kind):
        vals = rng.integers(0, P, n, dtype=np.uint64)
        pick = rng.integers(0, 16, n)
        vals = np.where(pick == 0, np.asarray(EDGES, dtype=np.uint64)[np.arange(n) % len(EDGES)], vals)
        if kind == "zero":
            vals[:] = 0
        elif kind == "sparse":
            vals[rng.integers(0, 8, n) == 0] = 0
        return vals
    ext = [np.stack([column("any"), column("sparse"), column("sparse")]), np.stack([column("sparse"), column("zero"), column("zero")]),
           np.stack([column("sparse"), column("sparse"), column("zero")])]
    base = [column("any") for _ in range(5)]
    return [ext[0], base[0], base[1], ext[1], base[2], ext[2], base[3], base[4]], rng


@pytest.mark.parametrize("salted", [True, False])
@pytest.mark.parametrize("n", FOUR_SIZES)
def test_ragged_trees_of_zipped_rows(n, salted):
    """bfs_merkle_build_rows: row_pattern_kernel + row_leaves_kernel (the template interpreter) on rows of many patterns"""
    _lib, lib, device = _lib_and_device()
    columns, rng = _mixed_columns(n, n + salted)
    bufs, rc = _row_columns(_lib, columns)
    salts = rng.integers(0, 256, 24 * n, dtype=np.uint8).tobytes()
    keep = ctypes.create_string_buffer(salts, len(salts))
    nodes = _nodes_for(n)
    _lib.check(lib.bfs_merkle_build_rows(rc, len(columns), n, ctypes.cast(keep, ctypes.c_void_p) if salted else None, 0, nodes.ptr, 0))
    device.synchronize(0)
    found = cc.interesting_rows([c for c in columns if c.ndim == 2], [c for c in columns if c.ndim == 1])
    rows = _rows_for(n, ROW_GROUP, n, cc.rows_of(found))
    patterns = {cc.row_pattern([c for c in columns if c.ndim == 2], i) for i in list(rows)[:2000]}
    assert len(patterns) >= 8
    _assert_none(_tree_failures(nodes, n, rows, lambda i: cc.row_preimage(columns, i, salts[24 * i:24 * i + 24] if salted else None),
                                "rows %d %s" % (n, "salted" if salted else "unsalted")))


def test_zipped_rows_of_a_range_of_longer_columns():
    """bfs_merkle_build_rows_range: 100003 rows from row 500 of columns of 101003 elements (limb planes limb_stride > n apart)"""
    _lib, lib, device = _lib_and_device()
    n, first, total = 100003, 500, 101003
    columns, rng = _mixed_columns(total, 77)
    bufs, rc = _row_columns(_lib, columns, offset=first)
    salts = rng.integers(0, 256, 24 * n, dtype=np.uint8).tobytes()
    keep = ctypes.create_string_buffer(salts, len(salts))
    nodes = _nodes_for(n)
    _lib.check(lib.bfs_merkle_build_rows_range(rc, len(columns), n, total, ctypes.cast(keep, ctypes.c_void_p), 0, nodes.ptr, 0))
    device.synchronize(0)
    window = [np.ascontiguousarray(c[..., first:first + n]) for c in columns]
    _assert_none(_tree_failures(nodes, n, range(n), lambda i: cc.row_preimage(window, i, salts[24 * i:24 * i + 24]), "rows range"))


def test_extension_elements_2p22_with_planted_waves():
    """bfs_merkle_build_xfe on 2^22 elements: waves (64 leaves) uniform of each class -- zero elements, lifted base elements,
    two-coefficient elements -- mixed waves, and mixed first and last waves"""
    import stark_brainfuck_amd as sb
    _lib, lib, device = _lib_and_device()
    n = 1 << 22
    soa = oracle.felt_array(0xC22, 0, 3 * n).reshape(3, n)
    planted = []
    for wave, kind in ((10, 0), (11, 1), (12, 2), (40000, 0), (40001, 1), (65535, 2), (n // 64 - 3, 1)):
        rows = range(64 * wave, 64 * wave + 64)
        if kind == 0:
            soa[:, rows] = 0
        elif kind == 1:
            soa[1:, rows] = 0
        else:
            soa[2, rows] = 0
        planted += rows
    for wave in (0, 13, 32768, 50001, n // 64 - 1):
        rows = list(range(64 * wave, 64 * wave + 64))
        _plant_elements(soa, rows)
        planted += rows
    arr = sb.XArray.from_numpy(soa)
    nodes = _nodes_for(n)
    _lib.check(lib.bfs_merkle_build_xfe(arr.ptr, arr.stride, n, nodes.ptr, 0))
    device.synchronize(0)
    assert np.array_equal(sb.Merkle(arr)._nodes.to_numpy(8, offset=8), nodes.to_numpy(8, offset=8))
    _assert_none(_tree_failures(nodes, n, cc.sample_rows(n, ELEMENT_GROUP, n, planted), lambda i: cc.xfe_preimage(soa, i), "xfe 2^22 planted"))


def test_base_elements_2p24_with_every_integer_width_at_wave_edges():
    """bfs_merkle_build_bfe on 2^24 values, the shape of bench.py's guard tree"""
    import stark_brainfuck_amd as sb
    _lib, lib, device = _lib_and_device()
    n = 1 << 24
    values = oracle.felt_array(0xB24, 0, n)
    planted = []
    for j, (name, lo, hi) in enumerate(cc.WIDTH_CLASSES):
        for wave in (j, 1000 * (j + 1), n // 64 - 1 - j):
            for i, v in ((64 * wave, lo), (64 * wave + 63, min(hi, P) - 1), (64 * wave + 64 if wave + 1 < n // 64 else 64 * wave + 1, lo + (hi - lo) // 3)):
                values[i] = np.uint64(v)
                planted.append(i)
    found = cc.interesting_rows([], [values])
    assert {name for _, name in found} == {name for name, _, _ in cc.WIDTH_CLASSES}
    arr = sb.BaseArray.from_numpy(values)
    nodes = _nodes_for(n)
    _lib.check(lib.bfs_merkle_build_bfe(arr.ptr, n, nodes.ptr, 0))
    device.synchronize(0)
    rows = cc.sample_rows(n, ELEMENT_GROUP, n, planted + cc.rows_of(found))
    _assert_none(_tree_failures(nodes, n, rows, lambda i: cc.bfe_preimage(values, i), "bfe 2^24 planted"))


LAYOUT1_VARIANTS = [(k7, k8) for k7 in (0, 1, 3) for k8 in (0, 1, 3)]      # stored coefficients of the two evaluation columns
GENERATED_CODES = {(1, 16): {0x3}, (9, 0): {0x3FFF | k7 << 14 | k8 << 16 for k7, k8 in LAYOUT1_VARIANTS}}    # csrc/rows_generated.hpp


@pytest.mark.parametrize("n_ext,n_base,variant", [(1, 16, None)] + [(9, 0, v) for v in LAYOUT1_VARIANTS] + [(9, 0, "quarters")])
def test_generated_row_layouts_2p20_with_planted_patterns(n_ext, n_base, variant):
    """the prover's two column layouts at 2^20 rows.  A launch of row_leaves_generated_kernel takes ONE pattern of its layout -- the
    first of the patterns present that the header has a variant for -- and leaves every other row to the interpreter launched
    behind it.  So each of Layout1's nine variants (0, 1 or 3 stored coefficients in each of the two evaluation columns; the parity
    test's list and the two it leaves out) gets a tree of its own in which it is the pattern of all rows but those of four
    workgroups, and no planted pattern is one the header knows: the dominant pattern is the one the straight-line kernel runs.
    "quarters" is the opposite mix: four variants a quarter of the rows each, one through the generated kernel, 3/4 of the rows
    through the interpreter."""
    _lib, lib, device = _lib_and_device()
    n = 1 << 20
    rng = np.random.default_rng(2000 + n_ext + 7 * LAYOUT1_VARIANTS.index(variant) if isinstance(variant, tuple) else 2000 + n_ext)
    ext = [rng.integers(1, P, (3, n), dtype=np.uint64) for _ in range(n_ext)]
    base = [rng.integers(0, P, n, dtype=np.uint64) for _ in range(n_base)]
    planted = []
    expected = 4 ** min(n_ext, 7) - 1                 # three stored coefficients in every column but the evaluation columns
    if isinstance(variant, tuple):
        k7, k8 = variant
        ext[7][k7:] = 0                               # the whole column: zero, a base-field constant, or full
        ext[8][k8:] = 0
        expected |= k7 << 14 | k8 << 16
    elif variant == "quarters":
        ext[7][:, n // 2:] = 0
        ext[8][1:, n // 4:3 * n // 4] = 0

    def group(g):
        rows = np.arange(ROW_GROUP * g, ROW_GROUP * g + ROW_GROUP)
        planted.extend(rows.tolist())
        return rows
    # the planted patterns change a column the header has no variant for: they all go to the interpreter
    rows = group(5)
    ext[0][2, rows[::2]] = 0                          # two stored coefficients, every other row of one workgroup
    rows = group(2000)
    ext[min(1, n_ext - 1)][:, rows] = 0               # a whole workgroup of zero elements
    rows = group(n // ROW_GROUP - 1)
    ext[0][1:, rows[1::3]] = 0                        # lifted base elements and two-coefficient elements in the last workgroup
    ext[2 % n_ext][2, rows[2::3]] = 0
    rows = group(0)
    for c in base[:3] + [e[k] for e in ext[:2] for k in range(2)]:
        c[rows[::5]] = np.asarray(EDGES, dtype=np.uint64)[np.arange(len(rows[::5])) % len(EDGES)]
    # what the data says about the launch: which patterns occur, and which of them the header has a kernel for
    code = np.zeros(n, dtype=np.int64)
    for c, e in enumerate(ext):
        code |= cc.stored_coefficients(e).astype(np.int64) << (2 * c)
    codes, counts = np.unique(code, return_counts=True)
    known = sorted(set(codes.tolist()) & GENERATED_CODES[(n_ext, n_base)])
    _note("generated layout %d+%d %s: patterns (code: rows) %s, with a generated variant: %s"
          % (n_ext, n_base, variant, {hex(c): k for c, k in zip(codes.tolist(), counts.tolist())}, [hex(c) for c in known]))
    assert len(codes) >= 3, "a second and a third pattern are planted"
    if variant == "quarters":
        assert len(known) == 4 and counts.max() < n // 4 + 1
    else:
        assert known == [expected], "the dominant pattern is the only one with a straight-line kernel"
        assert int(codes[np.argmax(counts)]) == expected and counts.max() >= n - 3 * ROW_GROUP
    columns = ext + base
    bufs, rc = _row_columns(_lib, columns)
    salts = rng.integers(0, 256, 24 * n, dtype=np.uint8).tobytes()
    keep = ctypes.create_string_buffer(salts, len(salts))
    sampled = cc.sample_rows(n, ROW_GROUP, n + n_ext, planted)
    for attempt in ("first", "remembered patterns"):
        nodes = _nodes_for(n)
        before = lib.bfs_row_generated_launches()
        _lib.check(lib.bfs_merkle_build_rows(rc, len(columns), n, ctypes.cast(keep, ctypes.c_void_p), 0, nodes.ptr, 0))
        device.synchronize(0)
        assert lib.bfs_row_generated_launches() > before, attempt
        _assert_none(_tree_failures(nodes, n, sampled, lambda i: cc.row_preimage(columns, i, salts[24 * i:24 * i + 24]),
                                    "generated layout %d+%d %s, %s" % (n_ext, n_base, variant, attempt)))
        del nodes


# ------------------------------------------------------------------------------------------------ (d) two code paths, every leaf
@pytest.mark.parametrize("name", ["nested32", "nested64"])
def test_row_leaf_implementations_agree_on_every_leaf(name):
    """Sampling cannot see a wrong digest at an unsampled row if the parents were built from it.  The row leaves have two
    implementations and a switch each, read once per process: the same proof bytes from the same stream with the straight-line
    kernels off, with the speculation on remembered patterns off, and with neither mean the same roots, hence every leaf of both
    row trees agrees between the generated kernels and the template interpreter.  One child process at a time, each bounded."""
    child = os.path.join(ROOT, "tests", "prove_digest_child.py")
    lines = {}
    for setting in ("", "BFS_ROWS_GENERATED", "BFS_ROWS_SPECULATE"):
        env = {k: v for k, v in os.environ.items() if k not in ("BFS_ROWS_GENERATED", "BFS_ROWS_SPECULATE")}
        if setting:
            env[setting] = "0"
        res = subprocess.run([sys.executable, child, name], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert res.returncode == 0, "%s=0\n%s\n%s" % (setting, res.stdout[-3000:], res.stderr[-3000:])
        line = [l for l in res.stdout.splitlines() if l.startswith("proof ")][-1].split()
        lines[setting] = line
        _note(setting or "default", " ".join(line))
    digests = {setting: line[line.index("sha256") + 1] for setting, line in lines.items()}
    launches = {setting: int(line[-1]) for setting, line in lines.items()}
    assert len(set(digests.values())) == 1, digests
    assert launches["BFS_ROWS_GENERATED"] == 0 and launches[""] > 0 and launches["BFS_ROWS_SPECULATE"] > 0, launches
