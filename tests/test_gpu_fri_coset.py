"""FRI with one Merkle leaf per folding coset on the GPU (Fri(..., folding_factor=a, coset_leaves=True), CosetMerkle,
bfs_merkle_build_xfe_cosets, bfs_fri_session_set_coset_leaves), bit for bit against a CPython model of the protocol
(tests/fri_coset_model.py) and against hashlib over oracle.dumps of every tuple.  Integer arithmetic and byte hashing throughout: no
tolerance anywhere."""
import ctypes
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import fri_coset_model as model
import fri_folding_model as per_element

pytestmark = pytest.mark.gpu

SEED = 0xC05E
OFFSET = 7
P = (1 << 64) - (1 << 32) + 1
BFS_ERR_BAD_ARG = 6
# the tree above q coset leaves is merkle.hip's (merkle_inner_launch): up to TOP_ONLY_MAX leaves one launch behind the leaf kernel
# (merkle_top_quad_kernel); from there to SUBTREE_LEAVES_MAX = 2 * SUBTREE_PARENTS_MAX leaves, that size included, nine-level subtree
# launches first (merkle_subtree_quad_kernel); above it -- q >= 2^18 -- a launch per level (merkle_parents_kernel) down to a level of
# SUBTREE_PARENTS_MAX parents
TOP_ONLY_MAX = 512
SUBTREE_PARENTS_MAX = 65536
SUBTREE_LEAVES_MAX = 2 * SUBTREE_PARENTS_MAX


@pytest.fixture(scope="module")
def sb():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import stark_brainfuck_amd
    from stark_brainfuck_amd import _lib
    _lib.load()            # raises BackendUnavailable if the HIP library is missing: no fallback
    return stark_brainfuck_amd


def _fri(sb, N, expansion, t, a, coset=True, XF=None):
    XF = sb.ExtensionField.main() if XF is None else XF
    BF = XF.modulus.coefficients[0].field
    assert BF.generator().value == OFFSET
    if coset is None:
        return sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, expansion, t, XF, folding_factor=a)
    return sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, expansion, t, XF, folding_factor=a, coset_leaves=coset)


def _by_rows(sb):
    from stark_brainfuck_amd import _lib
    return _lib.load().bfs_coset_trees_by_rows()


def _xarray(sb, soa, n):
    """an XArray of the first n elements of a (3, stride) array, the limb planes stride apart"""
    from stark_brainfuck_amd.device import DeviceBuffer
    soa = np.ascontiguousarray(soa, dtype=np.uint64)
    return sb.XArray(DeviceBuffer.from_numpy(soa.reshape(-1)), n, stride=soa.shape[1])


# ------------------------------------------------------------------------------------------------ 1. stand-alone coset trees
def _check_tree(sb, oracle, cw, n, a):
    tree = sb.CosetMerkle(_xarray(sb, cw, n), a)
    q = n // a
    assert tree.num_leafs == q and tree.coset_size == a and tree.depth == q.bit_length() - 1
    want = model.tree_nodes(oracle, cw, n, a)
    raw = tree._nodes.to_numpy(2 * q * 8).tobytes()
    got = [raw[64 * i:64 * i + 64] for i in range(2 * q)]
    wrong = [i for i in range(1, 2 * q) if got[i] != want[i]]
    assert wrong == [], "%d of %d nodes differ, first at heap index %d (leaves start at %d)" % (len(wrong), 2 * q - 1, wrong[0], q)
    assert tree.root() == want[1]
    return tree


@pytest.mark.parametrize("a", [2, 4, 8])
@pytest.mark.parametrize("q", [None, 2 * TOP_ONLY_MAX], ids=["n1024", "q1024"])
@pytest.mark.parametrize("planted", [None, "full", "short"], ids=["random", "full", "short"])
def test_coset_tree_against_hashlib(sb, oracle, a, q, planted):
    """every leaf and every parent.  n = 2^10 (q = 512, 256, 128: the top kernel alone) and q = 1024, just above it (a subtree launch
    first); random elements, planted one- to nine-byte limbs at wave and workgroup edges (the coset kernel hashes every leaf), and
    planted elements of 0, 1 and 2 coefficients (the tree goes through the zipped-row encoder)"""
    n = 1 << 10 if q is None else a * q
    assert (n // a <= TOP_ONLY_MAX) == (q is None)
    cw = model.tree_codeword(oracle, SEED + n + a, n, a, planted=planted)
    before = _by_rows(sb)
    tree = _check_tree(sb, oracle, cw, n, a)
    assert _by_rows(sb) - before == (1 if planted == "short" else 0)
    # open / verify / leafs of the Python mirror
    leaves = tree.leafs
    assert len(leaves) == n // a and all(len(t) == a for t in leaves[:3])
    for row in (0, n // a - 1, 65 % (n // a)):
        assert [[c.value for c in e.polynomial.coefficients] for e in leaves[row]] == \
            [oracle.xtrim([int(cw[y, row + j * (n // a)]) for y in range(3)]) for j in range(a)]
        path = tree.open(row)
        assert len(path) == tree.depth and sb.CosetMerkle.verify(tree.root(), row, path, leaves[row]) is True
        assert sb.CosetMerkle.verify(tree.root(), row ^ 1, path, leaves[row]) is False


@pytest.mark.parametrize("a", [2, 4, 8])
def test_coset_tree_of_a_codeword_with_a_stride_longer_than_its_length(sb, oracle, a):
    n = 1 << 10
    cw = model.tree_codeword(oracle, SEED + 77 + a, n, a, stride=n + 37, planted="full")
    before = _by_rows(sb)
    _check_tree(sb, oracle, cw, n, a)
    assert _by_rows(sb) == before
    # and from a list of elements: the same tree
    XF = sb.ExtensionField.main()
    elements = [XF.from_limbs([int(cw[y, i]) for y in range(3)]) for i in range(n)]
    tree = sb.CosetMerkle(elements, a)
    assert tree.root() == model.tree_nodes(oracle, cw, n, a)[1]
    assert tree.leafs[3][1] is elements[3 + n // a]


def _rows_tree(sb, cw, q, a):
    """the same tree by the zipped-row interpreter (bfs_merkle_build_rows_range: a extension columns that are slices of the codeword,
    q apart, unsalted) -- another encoder than the coset kernel's, itself checked against hashlib by the suites of the row commitments"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer
    cols = (_lib.RowColumn * a)(*[_lib.RowColumn(cw.ptr + 8 * j * q, 1, 0) for j in range(a)])
    nodes = DeviceBuffer(2 * q * 8)
    _lib.check(_lib.load().bfs_merkle_build_rows_range(cols, a, q, cw.stride, None, 0, nodes.ptr, 0))
    _lib.check(_lib.load().bfs_stream_synchronize(0))
    return nodes.to_numpy(2 * q * 8)


def _check_large_tree(sb, oracle, nodes, cw, host, q, a, seed):
    """a tree too large to pickle every tuple in CPython within a test's time (2^18 tuples: 10 to 40 s).  nodes: the 2 q digests from
    the GPU; cw / host: the codeword of a q elements in HBM and on the host.  Every parent is hashlib's hash of its two children as the
    GPU wrote them; 2 000 pseudo-random leaves and those at the edges of the first and the last workgroups are hashlib's over oracle.dumps
    of the tuple; and every node equals the zipped-row interpreter's."""
    raw = nodes.tobytes()
    assert len(raw) == 2 * q * 64
    wrong = [i for i in range(1, q) if hashlib.blake2b(raw[128 * i:128 * i + 128]).digest() != raw[64 * i:64 * i + 64]]
    assert wrong == [], "%d of %d parents differ from blake2b of their children, first at heap index %d" % (len(wrong), q - 1, wrong[0])
    rows = sorted(set(model.EDGE_ROWS) | {q - 1 - r for r in model.EDGE_ROWS} | {int(r) for r in np.random.RandomState(seed).randint(0, q, 2000)})
    for row in rows:
        tup = tuple(oracle.make_xfe([int(host[y, row + j * q]) for y in range(3)]) for j in range(a))
        assert raw[64 * (q + row):64 * (q + row) + 64] == hashlib.blake2b(oracle.dumps(tup)).digest(), "leaf %d" % row
    differ = np.flatnonzero((nodes.reshape(2 * q, 8)[1:] != _rows_tree(sb, cw, q, a).reshape(2 * q, 8)[1:]).any(axis=1)) + 1
    assert differ.size == 0, "%d nodes differ from the zipped-row encoder's, first at heap index %d (leaves start at %d)" % (differ.size, differ[0], q)


@pytest.mark.parametrize("a", [2, 4, 8])
def test_coset_tree_just_above_the_subtree_launch(sb, oracle, a):
    """q = 2^18 = 2 * SUBTREE_LEAVES_MAX, the smallest tree whose lowest level of parents (2^17 of them) is beyond the subtree kernel:
    merkle_parents_kernel hashes the coset leaves, the subtree launches start one level up.  Random elements with planted one- to
    nine-byte limbs at the edges."""
    q = 2 * SUBTREE_LEAVES_MAX
    assert q // 2 > SUBTREE_PARENTS_MAX and q // 4 <= SUBTREE_PARENTS_MAX
    n = a * q
    host = model.tree_codeword(oracle, SEED + 18 + a, n, a, planted="full")
    cw = _xarray(sb, host, n)
    before = _by_rows(sb)
    tree = sb.CosetMerkle(cw, a)
    assert _by_rows(sb) == before
    assert tree.num_leafs == q and tree.depth == 18
    nodes = tree._nodes.to_numpy(2 * q * 8)
    _check_large_tree(sb, oracle, nodes, cw, host, q, a, SEED + a)
    assert tree.root() == nodes[8:16].tobytes()
    row = q - 65
    tup = tuple(oracle.make_xfe([int(host[y, row + j * q]) for y in range(3)]) for j in range(a))
    assert oracle.merkle_verify(tree.root(), row, tree.open(row), oracle.dumps(tup))


def test_coset_tree_argument_checks(sb, oracle):
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer
    lib = _lib.load()
    cw = sb.XArray.from_numpy(model.tree_codeword(oracle, SEED, 64, 2))
    nodes = DeviceBuffer(2 * 64 * 8)
    for log2_coset in (0, 4):
        assert lib.bfs_merkle_build_xfe_cosets(cw.ptr, 64, 64, log2_coset, nodes.ptr, 0) == BFS_ERR_BAD_ARG
        assert b"log2_coset" in lib.bfs_last_error()
    assert lib.bfs_merkle_build_xfe_cosets(cw.ptr, 64, 48, 1, nodes.ptr, 0) == BFS_ERR_BAD_ARG         # not a power of two
    assert lib.bfs_merkle_build_xfe_cosets(cw.ptr, 64, 4, 3, nodes.ptr, 0) == BFS_ERR_BAD_ARG          # shorter than a coset
    assert lib.bfs_merkle_build_xfe_cosets(cw.ptr, 32, 64, 1, nodes.ptr, 0) == BFS_ERR_BAD_ARG         # stride < n
    assert lib.bfs_merkle_build_xfe_cosets(cw.ptr, 64, 64, 1, nodes.ptr + 8, 0) == BFS_ERR_BAD_ARG     # alignment
    assert lib.bfs_merkle_build_xfe_cosets(cw.ptr, 64, 8, 3, nodes.ptr, 0) == 0                        # a single leaf: the root is the leaf
    elements = [oracle.make_xfe([int(v) for v in cw.to_numpy()[:, i]]) for i in range(8)]
    assert nodes.to_numpy(8, offset=8).tobytes() == hashlib.blake2b(oracle.dumps(tuple(elements))).digest()


# ------------------------------------------------------------------------------------------------ 2. Fri.prove against the model
@functools.lru_cache(maxsize=None)
def _reference(N, expansion, t, a, prepushed=False, lifted=False):
    """the model's proof of the seeded codeword -- computed once per case, shared, never changed"""
    from oracle import ref_oracle as o
    omega = o.primitive_nth_root(N)
    if lifted:       # a polynomial with base-field coefficients: every element of C_0 stores one coefficient (or none)
        d = N // expansion
        coeffs = np.zeros((3, d), dtype=np.uint64)
        coeffs[0] = o.felt_array(SEED + N, 0, d)
        cw = o.xevaluate_soa(coeffs, OFFSET, omega, N)
        assert not cw[1:].any()
    else:
        cw = model.codeword_of(o, SEED + N + expansion, N, expansion, OFFSET, omega)
    ps = o.ProofStreamOracle()
    if prepushed:
        for obj in _prepushed(lambda limbs: o.make_xfe(limbs), o):
            ps.push(obj)
    out = model.prove(o, cw, OFFSET, omega, expansion, t, a, proof_stream=ps)
    out["bytes"] = ps.serialize()
    out["codeword"] = cw
    return out


def _prepushed(make_element, oracle):
    """objects in front of the proof -- a digest, a tuple of elements, a list of digests -- with enough digests (6.4 KB) that the native
    prover's Fiat-Shamir look-ahead takes them as its prefix"""
    digests = [hashlib.blake2b(bytes([i])).digest() for i in range(101)]
    elements = [make_element([oracle.felt(SEED + 88, 3 * i + j) for j in range(3)]) for i in range(3)]
    return [digests[0], tuple(elements), digests[1:]]


# (a, N, expansion, t)
PROVE_CASES = [(2, 1 << 6, 16, 4), (2, 1 << 6, 4, 4), (2, 1 << 9, 4, 4), (2, 1 << 14, 16, 8),
               (4, 1 << 5, 4, 4), (4, 1 << 10, 4, 4), (4, 1 << 12, 4, 4), (4, 1 << 16, 4, 4),
               (8, 1 << 6, 4, 4), (8, 1 << 10, 16, 4), (8, 1 << 13, 4, 4), (8, 1 << 17, 4, 4)]


# commits too large for a model transcript (it would pickle every tuple): test_commit_of_a_large_codeword
LARGE_COMMIT_CASES = [(2, 1 << 18, 4, 4), (2, 1 << 20, 4, 4)]


def _coset_rounds(cases):
    """{(a, round is produced by a fold, leaves of its tree)} over the coset rounds (every round but the last) of the cases"""
    return {(a, r > 0, N >> (k * (r + 1))) for a, N, e, _ in cases for k in [a.bit_length() - 1] for r in range(model.num_folds(N, e, k))}


def test_prove_cases_put_a_round_on_every_kernel_and_every_threshold_side():
    """two kernels per folding factor -- coset_leaves_kernel<0, a> reads round 0's codeword, coset_leaves_kernel<k, a> folds the later
    rounds' on the way -- and the tree above their q leaves is one launch up to TOP_ONLY_MAX leaves, subtree launches up to
    SUBTREE_LEAVES_MAX, a launch per level first above that; a single workgroup (q <= 64) and a partly filled one (q < 64) are sides of
    their own.  One fold only (the round behind round 0 is the last, per-element one) and several.  The side above SUBTREE_LEAVES_MAX
    is a property of merkle.hip's levels, not of the leaf kernel: one folding factor has to reach it from a codeword that is read
    and from one that is folded (the stand-alone trees reach it for every a)."""
    rounds = _coset_rounds(PROVE_CASES)
    for a in (2, 4, 8):
        for folded in (False, True):
            sizes = {q for a_, f, q in rounds if a_ == a and f == folded}
            assert any(q < 64 for q in sizes) and any(64 < q <= TOP_ONLY_MAX for q in sizes) and any(TOP_ONLY_MAX < q <= SUBTREE_LEAVES_MAX for q in sizes), (a, folded, sizes)
        folds = {model.num_folds(N, e, a.bit_length() - 1) for a_, N, e, _ in PROVE_CASES if a_ == a}
        assert 1 in folds and max(folds) >= 3, (a, folds)
    large = _coset_rounds(LARGE_COMMIT_CASES)
    for folded in (False, True):
        sizes = {q for _, f, q in large if f == folded}
        assert SUBTREE_LEAVES_MAX in sizes and any(q > SUBTREE_LEAVES_MAX for q in sizes), (folded, sizes)      # the threshold itself and above it


@pytest.mark.parametrize("a,N,expansion,t", PROVE_CASES)
def test_prove_is_the_model_byte_for_byte(sb, a, N, expansion, t):
    ref = _reference(N, expansion, t, a)
    fri = _fri(sb, N, expansion, t, a)
    assert fri.num_rounds() == ref["rounds"]
    cw = sb.XArray.from_numpy(ref["codeword"])
    ps = sb.ProofStream()
    before = _by_rows(sb)
    assert fri.prove(cw, ps) == ref["indices"]
    assert _by_rows(sb) == before, "a round of a codeword of full elements went through the zipped-row encoder"
    assert len(ps.objects) == len(ref["proof_stream"].objects)
    assert ps.serialize() == ref["bytes"]
    vs = sb.ProofStream()
    vs.objects = list(ps.objects)
    assert fri.verify(vs, ref["roots"][0]) is True
    assert vs.read_index == len(vs.objects)
    assert sb.ProofStream().deserialize(ref["bytes"]).objects is not None and fri.verify(sb.ProofStream().deserialize(ps.serialize()), ref["roots"][0]) is True
    if (a, N) in ((2, 1 << 9), (4, 1 << 12), (8, 1 << 13)):
        bad = sb.ProofStream()
        bad.objects = list(ps.objects)
        bad.objects[0] = bytes(64)           # a wrong round-1 root changes every later challenge
        assert fri.verify(bad, ref["roots"][0]) is False
        # the per-element verifier does not take the stream: by 4 and 8 it answers False; by 2 it is the reference's, which unpacks
        # three values from a tuple of two and raises
        plain = _fri(sb, N, expansion, t, a, coset=False)
        if a == 2:
            with pytest.raises(ValueError):
                plain.verify(sb.ProofStream().deserialize(ref["bytes"]), ref["roots"][0])
        else:
            assert plain.verify(sb.ProofStream().deserialize(ref["bytes"]), ref["roots"][0]) is False


@pytest.mark.parametrize("a", [2, 4, 8])
def test_prove_on_a_codeword_lifted_from_the_base_field(sb, a):
    """round 0's tuples hold elements of one coefficient: its tree is the zipped-row encoder's; the folded rounds are full again"""
    N, expansion, t = 1 << 9, 4, 4
    ref = _reference(N, expansion, t, a, lifted=True)
    fri = _fri(sb, N, expansion, t, a)
    ps = sb.ProofStream()
    before = _by_rows(sb)
    assert fri.prove(sb.XArray.from_numpy(ref["codeword"]), ps) == ref["indices"]
    assert _by_rows(sb) - before == 1
    assert ps.serialize() == ref["bytes"]
    assert fri.verify(sb.ProofStream().deserialize(ps.serialize()), ref["roots"][0]) is True


def test_commit_and_query_are_the_python_mirror_of_prove(sb):
    """Fri.commit's trees are CosetMerkle views on the session's nodes; query / query_last push what prove pushes"""
    a, N, expansion, t = 4, 1 << 10, 4, 4
    ref = _reference(N, expansion, t, a)
    fri = _fri(sb, N, expansion, t, a)
    ps = sb.ProofStream()
    codewords, trees = fri.commit(sb.XArray.from_numpy(ref["codeword"]), ps)
    F = ref["rounds"] - 1
    assert len(codewords) == F + 1 and len(trees) == F and all(isinstance(tree, sb.CosetMerkle) for tree in trees)
    assert [tree.root() for tree in trees] == ref["roots"][:F]
    assert [tree.num_leafs for tree in trees] == [N >> (2 * (r + 1)) for r in range(F)]
    top = fri.sample_indices(ps.prover_fiat_shamir(), len(codewords[1]), len(codewords[-1]), t)
    assert top == ref["indices"]
    for i in range(F - 1):
        opened = fri.query(trees[i], trees[i + 1], [x % trees[i].num_leafs for x in top], ps)
        assert len(opened) == a * t
    fri.query_last(trees[-1], codewords[-1], [x % trees[-1].num_leafs for x in top], ps)
    assert ps.serialize() == ref["bytes"]


# ------------------------------------------------------------------------------------------------ 3. commits at 2^18 and 2^20
@pytest.mark.parametrize("a,N,expansion,t", LARGE_COMMIT_CASES, ids=["2p18", "2p20"])
def test_commit_of_a_large_codeword(sb, oracle, a, N, expansion, t):
    """folding by 2.  At 2^18 round 0's tree has 2^17 = SUBTREE_LEAVES_MAX leaves, the largest that starts with a subtree launch; at 2^20
    rounds 0 and 1 have 2^19 and 2^18, so merkle_parents_kernel runs above the leaves of coset_leaves_kernel<0, 2> and of
    coset_leaves_kernel<1, 2>.  Every round's codeword against oracle.fri_fold.  The trees of 2^16 to 2^18 leaves as
    _check_large_tree says (every parent and sampled leaves against hashlib, every node against the zipped-row encoder); every other
    root against the stand-alone tree of the same codeword -- the same leaf kernel, so that shows the driver, not the encoder -- and
    four paths of rounds 0 and 1 against hashlib.  (No model transcript here: it would pickle every tuple.)"""
    k = a.bit_length() - 1
    omega = oracle.primitive_nth_root(N)
    soa = model.codeword_of(oracle, SEED + N.bit_length(), N, expansion, OFFSET, omega)
    fri = _fri(sb, N, expansion, t, a)
    cw = sb.XArray.from_numpy(soa)
    ps = sb.ProofStream()
    before = _by_rows(sb)
    codewords, trees = fri.commit(cw, ps)
    F = model.num_folds(N, expansion, k)
    assert fri.num_rounds() == F + 1 == len(codewords) and len(trees) == F
    assert [len(c) for c in codewords] == [N >> (k * r) for r in range(F + 1)]
    host = [c.array.to_numpy() for c in codewords]
    assert np.array_equal(host[0], soa)
    roots = [tree.root() for tree in trees] + [sb.Merkle(codewords[-1].array).root()]
    hashed = 0
    for r in range(F):
        q = len(codewords[r]) // a
        assert trees[r].num_leafs == q
        if SUBTREE_LEAVES_MAX // 2 <= q <= 2 * SUBTREE_LEAVES_MAX:
            _check_large_tree(sb, oracle, trees[r]._nodes.to_numpy(2 * q * 8), codewords[r].array, host[r], q, a, SEED + r)
            hashed += 1
        else:
            assert sb.CosetMerkle(codewords[r].array, a).root() == roots[r], "round %d" % r
    assert hashed >= 2
    assert _by_rows(sb) == before
    assert [bytes(x) for x in ps.objects[:F]] == roots[1:] and len(ps.objects) == F + 1
    mirror = oracle.ProofStreamOracle()
    g, w = OFFSET, omega
    for r in range(F):
        if r > 0:
            mirror.push(roots[r])
        alpha = oracle.xsample(mirror.prover_fiat_shamir())
        want, g, w = model.fold_round(oracle, host[r], alpha, g, w, k)
        assert np.array_equal(want, host[r + 1]), "codeword %d" % (r + 1)
    for r in (0, 1):
        q = len(codewords[r]) // a
        for row in (0, 63, 64, q - 1):
            tup = tuple(oracle.make_xfe([int(host[r][y, row + j * q]) for y in range(3)]) for j in range(a))
            assert oracle.merkle_verify(roots[r], row, trees[r].open(row), oracle.dumps(tup))
    root0 = roots[0]
    del codewords, trees
    ps2 = sb.ProofStream()
    top = fri.prove(cw, ps2)
    assert len(top) == t and all(0 <= i < N >> k for i in top)
    assert [bytes(x) for x in ps2.objects[:F]] == roots[1:]
    assert model.count_digests(ps2.objects) == t * sum((N >> (k * (i + 1))).bit_length() - 1 for i in range(F))
    vs = sb.ProofStream()
    vs.objects = list(ps2.objects)
    assert fri.verify(vs, root0) is True and vs.read_index == len(vs.objects)


# ------------------------------------------------------------------------------------------------ 4. switches and prior state
_CHILD = r"""
import hashlib, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import stark_brainfuck_amd as sb
import test_gpu_fri_coset as T
from oracle import ref_oracle as o
N, expansion, t = 1 << 10, 4, 4
XF = sb.ExtensionField.main()
cw = T.model.codeword_of(o, T.SEED + N + expansion, N, expansion, T.OFFSET, o.primitive_nth_root(N))
for a in (2, 8):
    for pre in (False, True):
        ps = sb.ProofStream()
        if pre:
            for obj in T._prepushed(XF.from_limbs, o):
                ps.push(obj)
        top = T._fri(sb, N, expansion, t, a, True, XF).prove(sb.XArray.from_numpy(cw), ps)
        print("RESULT", a, pre, top, hashlib.sha256(ps.serialize()).hexdigest())
"""


def test_prove_without_the_lookahead(sb):
    """the look-ahead switch is read once per process: BFS_FRI_LOOKAHEAD=0 gets a process of its own"""
    N, expansion, t = 1 << 10, 4, 4
    want = []
    for a in (2, 8):
        for pre in (False, True):
            ref = _reference(N, expansion, t, a, prepushed=pre)
            want.append("RESULT %s %s %s %s" % (a, pre, ref["indices"], hashlib.sha256(ref["bytes"]).hexdigest()))
    env = dict(os.environ)
    env["BFS_FRI_LOOKAHEAD"] = "0"
    res = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:]
    assert [line for line in res.stdout.splitlines() if line.startswith("RESULT")] == want


@pytest.mark.parametrize("a,N", [(2, 1 << 10), (4, 1 << 12), (8, 1 << 10)])
def test_prove_behind_objects_pushed_beforehand(sb, oracle, a, N):
    """the stream already holds objects (6.5 KB of them: the Fiat-Shamir look-ahead engages and has to count F - 1 coming roots)"""
    expansion, t = 4, 4
    ref = _reference(N, expansion, t, a, prepushed=True)
    XF = sb.ExtensionField.main()
    ps = sb.ProofStream()
    pre = _prepushed(XF.from_limbs, oracle)
    for obj in pre:
        ps.push(obj)
    fri = _fri(sb, N, expansion, t, a, XF=XF)
    assert fri.prove(sb.XArray.from_numpy(ref["codeword"]), ps) == ref["indices"]
    assert ps.serialize() == ref["bytes"]
    vs = sb.ProofStream()
    vs.objects, vs.read_index = list(ps.objects), len(pre)
    assert fri.verify(vs, ref["roots"][0]) is True


# ------------------------------------------------------------------------------------------------ 5. round0_tree
@pytest.mark.parametrize("a,N", [(2, 1 << 10), (4, 1 << 12), (8, 1 << 13)])
def test_a_proof_with_the_callers_round0_tree_is_the_same_proof(sb, a, N):
    expansion, t = 4, 4
    ref = _reference(N, expansion, t, a)
    fri = _fri(sb, N, expansion, t, a)
    cw = sb.XArray.from_numpy(ref["codeword"])
    tree = sb.CosetMerkle(cw, a)
    assert tree.root() == ref["roots"][0]
    ps = sb.ProofStream()
    assert fri.prove(cw, ps, round0_tree=tree) == ref["indices"]
    assert ps.serialize() == ref["bytes"]
    assert fri.verify(sb.ProofStream().deserialize(ps.serialize()), tree.root()) is True
    # the wrong kind, the wrong coset size, known_leafs
    other = 4 if a != 4 else 2
    for bad in (sb.Merkle(cw), sb.CosetMerkle(cw, other)):
        with pytest.raises(AssertionError, match="round0_tree"):
            fri.prove(cw, sb.ProofStream(), round0_tree=bad)
    with pytest.raises(AssertionError, match="known_leafs"):
        fri.prove(cw, sb.ProofStream(), known_leafs={0: cw.to_elements()[0]})
    with pytest.raises(AssertionError, match="CosetMerkle"):
        _fri(sb, N, expansion, t, a, coset=False).prove(cw, sb.ProofStream(), round0_tree=tree)
    # and the stream is untouched by a refused call
    ps3 = sb.ProofStream()
    with pytest.raises(AssertionError):
        fri.prove(cw, ps3, round0_tree=sb.Merkle(cw))
    assert ps3.objects == []


def test_session_argument_checks(sb, oracle):
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer
    from stark_brainfuck_amd.ip import NativeTranscript
    lib = _lib.load()
    N, expansion = 256, 4
    omega = oracle.primitive_nth_root(N)
    cw = sb.XArray.from_numpy(model.codeword_of(oracle, SEED, N, expansion, OFFSET, omega))
    coset_tree, plain_tree = sb.CosetMerkle(cw, 4), sb.Merkle(cw)

    def commit(k, coset, round0=None, expansion=expansion):
        session = lib.bfs_fri_session_new()
        try:
            assert lib.bfs_fri_session_set_folding(session, k) == 0
            assert lib.bfs_fri_session_set_coset_leaves(session, coset) == 0
            if round0 is not None:
                round0(session)
            transcript = NativeTranscript()
            rc = lib.bfs_fri_commit(session, transcript.handle, cw.ptr, cw.stride, 8, OFFSET, omega, expansion, 0)
            said = lib.bfs_last_error() if rc else b""
            if rc == 0:
                assert lib.bfs_fri_session_set_coset_leaves(session, 1 - coset) == BFS_ERR_BAD_ARG
                assert b"already committed" in lib.bfs_last_error()
                F = lib.bfs_fri_session_rounds(session) - 1
                want = [N >> (k * (r + 1)) if coset and r < F else N >> (k * r) for r in range(F + 1)]
                assert [lib.bfs_fri_session_round_leaves(session, r) for r in range(F + 2)] == want + [0]
                element = transcript.to_native(sb.ExtensionField.main().from_limbs([1, 2, 3]))
                rc_alias = lib.bfs_fri_session_alias(session, transcript.handle, 0, 0, element)
                assert rc_alias == (BFS_ERR_BAD_ARG if coset else 0)
                if coset:
                    assert b"cosets" in lib.bfs_last_error()
            return rc, said
        finally:
            lib.bfs_fri_session_free(session)

    for k in (1, 2, 3):
        assert commit(k, 1)[0] == 0 and commit(k, 0)[0] == 0
    # the caller's round-0 tree: the right one, one of another shape, one of the other kind
    assert commit(2, 1, lambda s: lib.bfs_fri_session_round0_coset_tree(s, coset_tree._nodes.ptr, 64, coset_tree.root()))[0] == 0
    rc, said = commit(1, 1, lambda s: lib.bfs_fri_session_round0_coset_tree(s, coset_tree._nodes.ptr, 64, coset_tree.root()))
    assert rc == BFS_ERR_BAD_ARG and b"leaves" in said
    rc, said = commit(2, 1, lambda s: lib.bfs_fri_session_round0_tree(s, plain_tree._nodes.ptr, plain_tree.root()))
    assert rc == BFS_ERR_BAD_ARG and b"leaves" in said
    rc, said = commit(2, 0, lambda s: lib.bfs_fri_session_round0_coset_tree(s, coset_tree._nodes.ptr, 64, coset_tree.root()))
    assert rc == BFS_ERR_BAD_ARG and b"leaves" in said
    session = lib.bfs_fri_session_new()
    assert lib.bfs_fri_session_round0_coset_tree(session, coset_tree._nodes.ptr, 48, coset_tree.root()) == BFS_ERR_BAD_ARG
    lib.bfs_fri_session_free(session)
    # fewer than one fold: folding by 2 tolerates it in the per-element mode only
    assert commit(1, 0, expansion=128)[0] == 0
    rc, said = commit(1, 1, expansion=128)
    assert rc == BFS_ERR_BAD_ARG and b"less than one fold" in said
    # bfs_fri_prove_cosets = a session with the flag; flag 0 = bfs_fri_prove_folded
    outs = []
    for call in ("cosets1", "cosets0", "folded"):
        transcript = NativeTranscript()
        top = (ctypes.c_uint64 * 4)()
        if call == "folded":
            _lib.check(lib.bfs_fri_prove_folded(transcript.handle, cw.ptr, cw.stride, 8, OFFSET, omega, expansion, 2, 4, top, 0))
        else:
            _lib.check(lib.bfs_fri_prove_cosets(transcript.handle, cw.ptr, cw.stride, 8, OFFSET, omega, expansion, 2, int(call[-1]), 4, top, 0))
        outs.append((list(top), transcript.serialize()))
    assert outs[1] == outs[2] and outs[0] != outs[1]
    fri = _fri(sb, N, expansion, 4, 4)
    ps = sb.ProofStream()
    assert fri.prove(cw, ps) == outs[0][0] and ps.serialize() == outs[0][1]


# ------------------------------------------------------------------------------------------------ 6. the default mode is untouched
@pytest.mark.parametrize("a,N", [(2, 1 << 10), (4, 1 << 10)])
def test_the_default_mode_after_a_coset_proof_is_the_per_element_model(sb, oracle, a, N):
    """coset_leaves=False (and a Fri built without the argument) in the same process, behind a coset-mode proof of the same codeword:
    the bytes of tests/fri_folding_model.py -- for a = 2 the reference's"""
    expansion, t = 4, 4
    ref = _reference(N, expansion, t, a)
    cw = sb.XArray.from_numpy(ref["codeword"])
    ps = sb.ProofStream()
    assert _fri(sb, N, expansion, t, a).prove(cw, ps) == ref["indices"] and ps.serialize() == ref["bytes"]
    old = per_element.prove(oracle, ref["codeword"], OFFSET, oracle.primitive_nth_root(N), expansion, t, a)
    if a == 2:
        theirs = oracle.fri_prove(ref["codeword"], OFFSET, oracle.primitive_nth_root(N), expansion, t)
        assert theirs["proof_stream"].serialize() == old["proof_stream"].serialize()
    for coset in (False, None):
        fri = _fri(sb, N, expansion, t, a, coset=coset)
        assert fri.coset_leaves is False
        ps = sb.ProofStream()
        assert fri.prove(cw, ps) == old["indices"]
        assert ps.serialize() == old["proof_stream"].serialize()
        assert fri.verify(sb.ProofStream().deserialize(ps.serialize()), old["roots"][0]) is True
    # and a coset proof again behind those
    ps = sb.ProofStream()
    assert _fri(sb, N, expansion, t, a).prove(cw, ps) == ref["indices"] and ps.serialize() == ref["bytes"]
