"""tests/commitment_check.py checked without a GPU: trees built by the oracle and laid out the way the device lays them out pass,
each planted fault is reported with its kind and nothing else, the FRI transcript assembled from trees is oracle.fri_prove's byte
for byte (and the reference's own, where a golden stream exists), and sample_rows holds what it promises."""
import hashlib

import numpy as np
import pytest

import commitment_check as cc
from conftest import golden_bytes, load_golden
from oracle import ref_oracle as oracle

SEED = 0x5EED
SIZES = [1, 2, 3, 64, 65, 1023, 1025, 4099]


def device_heap(tree, seed=1):
    """the nodes of a MerkleOracle in the device's layout: 64-byte slots, garbage where the device writes nothing (slot 0 and the
    leaf slots of absent leaves)"""
    npo2 = 1 << tree.depth
    heap = bytearray(np.random.default_rng(seed).integers(0, 256, cc.SLOT * 2 * npo2, dtype=np.uint8).tobytes())
    for k in range(1, npo2 + tree.num_leafs):
        assert len(tree.nodes[k]) == cc.SLOT
        heap[cc.SLOT * k:cc.SLOT * k + cc.SLOT] = tree.nodes[k]
    return heap


def xfe_codeword(n, seed):
    soa = oracle.felt_array(SEED + seed, 0, 3 * n).reshape(3, n)
    if n > 8:
        soa[:, 3] = 0
        soa[1:, 5] = 0
        soa[2, 6] = 0
        soa[0, 7] = 200
    return soa


def all_checks(heap, n, soa, rows=None):
    npo2, depth = cc.tree_shape(n)
    leaf_level = bytes(heap[cc.SLOT * npo2:cc.SLOT * (npo2 + n)])
    rows = range(n) if rows is None else rows
    return (cc.check_parents(cc.bytes_reader(heap), depth, n, chunk=256)
            + cc.check_leaves(cc.digest_reader(leaf_level), rows, lambda i: cc.xfe_preimage(soa, i)))


def flip(heap, k, bit=0):
    heap[cc.SLOT * k + bit // 8] ^= 1 << (bit % 8)


@pytest.mark.parametrize("n", SIZES)
def test_oracle_trees_in_device_layout_pass(n):
    soa = xfe_codeword(n, n)
    tree, _ = oracle.xfe_merkle(soa)
    assert cc.tree_shape(n) == (1 << tree.depth, tree.depth)
    assert all_checks(device_heap(tree), n, soa) == []
    # base-field leaves and byte-string leaves: the same tree rule, other preimages
    values = oracle.felt_array(SEED + 1, 0, n)
    tree = oracle.MerkleOracle([oracle.dumps(oracle.make_bfe(int(v))) for v in values])
    heap = device_heap(tree)
    npo2, depth = cc.tree_shape(n)
    assert cc.check_parents(cc.bytes_reader(heap), depth, n) == []
    assert cc.check_leaves(cc.digest_reader(bytes(heap[cc.SLOT * npo2:])), range(n), lambda i: cc.bfe_preimage(values, i)) == []


def test_chunked_reading_is_the_same_check():
    """a reader of uint64 words (DeviceBuffer.to_numpy's shape) and every chunk size see the same tree"""
    n = 4099
    soa = xfe_codeword(n, 9)
    heap = device_heap(oracle.xfe_merkle(soa)[0])
    words = np.frombuffer(bytes(heap), dtype=np.uint64)
    reader = cc.heap_reader(lambda count, offset: words[offset:offset + count])
    for chunk in (1, 7, 4096, 1 << 16):
        assert cc.check_parents(reader, 13, n, chunk=chunk) == []
    flip(heap, 4096 + 2049)                                  # the parent above the last present leaf
    words = np.frombuffer(bytes(heap), dtype=np.uint64)
    for chunk in (1, 7, 4096, 1 << 16):
        assert [m for _, m in cc.check_parents(reader, 13, n, chunk=chunk)][0].startswith("level 12 index 2049 ")


@pytest.mark.parametrize("n", [1025, 4099])
def test_each_fault_is_caught_with_its_kind(n):
    soa = xfe_codeword(n, n + 1)
    tree, _ = oracle.xfe_merkle(soa)
    good = device_heap(tree)
    npo2, depth = cc.tree_shape(n)

    def kinds_and_messages(heap, rows=None):
        failures = all_checks(heap, n, soa, rows)
        return {k for k, _ in failures}, [m for _, m in failures]

    deep = npo2 // 2 + 5                                     # a parent of two present leaves
    last = (npo2 + n - 1) // 2                               # the parent above the last present leaf
    childless = npo2 - 1                                     # both leaf slots absent
    for k, bit in ((deep, 0), (1, 511), (last, 77), (childless, 300), (37, 9)):
        heap = bytearray(good)
        flip(heap, k, bit)
        kinds, messages = kinds_and_messages(heap)
        assert kinds == {"parent"}
        level = k.bit_length() - 1
        named = {"level %d index %d " % (level, k - (1 << level))} | ({"level %d index %d " % (level - 1, k // 2 - (1 << (level - 1)))} if k > 1 else set())
        assert {m[:m.index("(")] for m in messages} == named      # the node itself and, stored child of it, its parent
    # a leaf digest: the leaf check names the row; the parent above it no longer matches either
    rows = cc.sample_rows(n, 64, seed=3)
    row = rows[len(rows) // 2]
    heap = bytearray(good)
    flip(heap, npo2 + row, 100)
    failures = all_checks(heap, n, soa, rows)
    assert [f for f in failures if f[0] == "leaf"] == [("leaf", "row %d (preimage of %d bytes)" % (row, len(cc.xfe_preimage(soa, row))))]
    assert [m[:m.index("(")] for k, m in failures if k == "parent"] == ["level %d index %d " % (depth - 1, row // 2)]
    # a leaf digest that is the digest of other data, parents built from it: only the leaf check can see it
    other = soa.copy()
    other[0, row] ^= np.uint64(1)
    heap = device_heap(oracle.xfe_merkle(other)[0])
    kinds, _ = kinds_and_messages(heap, rows)
    assert kinds == {"leaf"}
    assert all_checks(heap, n, soa, [r for r in rows if r != row]) == []
    # an absent leaf slot hashed as 64 zero bytes instead of 32
    wrong = oracle.MerkleOracle([cc.xfe_preimage(soa, i) for i in range(n)])
    for k in range(npo2 - 1, 0, -1):
        kids = [wrong.nodes[c] if c < npo2 + n else bytes(64) for c in (2 * k, 2 * k + 1)] if k >= npo2 // 2 else [wrong.nodes[2 * k], wrong.nodes[2 * k + 1]]
        wrong.nodes[k] = hashlib.blake2b(kids[0] + kids[1]).digest()
    kinds, messages = kinds_and_messages(device_heap(wrong))
    assert kinds == {"parent"}
    assert all(m.startswith("level %d " % (depth - 1)) or m.startswith("...") for m in messages)
    absent_parents = npo2 // 2 - n // 2                      # parents with at least one absent child
    assert len(cc.check_parents(cc.bytes_reader(device_heap(wrong)), depth, n)) == min(absent_parents, cc.MAX_REPORTED) + (absent_parents > cc.MAX_REPORTED)


def test_salted_rows_and_the_picked_copy():
    """row preimages as test_zipped_rows_commitment_on_device_vs_oracle builds them, through PickedRows"""
    n = 300
    rng = np.random.default_rng(5)
    ext = [rng.integers(0, oracle.P, (3, n), dtype=np.uint64) for _ in range(3)]
    ext[1][2, ::3] = 0
    ext[2][:, ::5] = 0
    base = [rng.integers(0, oracle.P, n, dtype=np.uint64) for _ in range(5)]
    base[0][::2] = 7
    columns = [ext[0], base[0], base[1], ext[1], base[2], ext[2], base[3], base[4]]
    salts = rng.integers(0, 256, 24 * n, dtype=np.uint8).tobytes()

    def orow(i):
        return tuple(oracle.make_xfe([int(c[0, i]), int(c[1, i]), int(c[2, i])]) if c.ndim == 2 else oracle.make_bfe(int(c[i])) for c in columns)
    pre = [oracle.salted_leaf_bytes(orow(i), salts[24 * i:24 * i + 24]) for i in range(n)]
    tree = oracle.MerkleOracle(pre)
    heap = device_heap(tree)
    rows = cc.sample_rows(n, 8, seed=1, uniform=32)
    picked = cc.PickedRows(rows)
    for c in columns:
        picked.pick(c)
    digests = cc.digest_reader(bytes(heap[cc.SLOT * 512:]))
    assert cc.check_leaves(digests, rows, lambda i: picked.preimage(i, salts[24 * i:24 * i + 24])) == []
    assert cc.check_leaves(digests, rows, lambda i: cc.row_preimage(columns, i, salts[24 * i:24 * i + 24])) == []
    assert {k for k, _ in cc.check_leaves(digests, rows[:5], lambda i: cc.row_preimage(columns, i))} == {"leaf"}      # (the salt forgotten)
    assert cc.row_pattern(ext, 1) == (3, 3, 3) and cc.row_pattern(ext, 0) == (3, 2, 0)


def test_interesting_rows_finds_every_class():
    n = 5000
    rng = np.random.default_rng(11)
    soa = rng.integers(1 << 63, oracle.P, (3, n), dtype=np.uint64)
    base = rng.integers(1 << 63, oracle.P, n, dtype=np.uint64)
    planted = {}
    for j, (name, lo, hi) in enumerate(cc.WIDTH_CLASSES):
        for v, at in ((lo, 100 + 10 * j), (min(hi, oracle.P) - 1, 101 + 10 * j)):
            base[at] = v
            soa[1, at] = v
            assert cc.width_class(v) == name and len(oracle.dumps(v)) == len(oracle.dumps(lo))
            planted.setdefault(name, []).append(at)
    soa[:, 1000] = 0
    soa[1:, 1001] = 0
    soa[2, 1002] = 0
    found = cc.interesting_rows([soa], [base], cap=5000)
    for name, rows in planted.items():
        assert set(rows) <= set(found[("b0", name)][1]) and set(rows) <= set(found[("x0.1", name)][1])
    assert found[("x0", "coefficients=0")] == (1, [1000]) and found[("x0", "coefficients=1")] == (1, [1001])
    assert found[("x0", "coefficients=2")] == (1, [1002]) and found[("x0", "coefficients=3")][0] == n - 3
    assert found[("x0.0", "int<2^8")] == (1, [1000])
    capped = cc.interesting_rows([soa], [base], cap=2)
    assert all(len(rows) <= 2 for _, rows in capped.values()) and capped[("b0", "long9")][0] == found[("b0", "long9")][0]
    assert set(cc.rows_of(capped)) >= {1000, 1001, 1002}
    assert cc.class_counts(found)["coefficients=0"] == (1, 1)


def _trees_of(codewords):
    """per round: (host codeword, device-layout heap), every one passed through the checks first"""
    heaps = []
    for cw in codewords[:-1]:
        n = cw.shape[1]
        heap = device_heap(oracle.xfe_merkle(cw)[0])
        assert all_checks(heap, n, cw, cc.sample_rows(n, 64, seed=n, uniform=64)) == []
        heaps.append(bytes(heap))
    return heaps


def _transcript(codewords, expansion, t, proof_stream=None):
    heaps = _trees_of(codewords)
    return cc.fri_transcript_from_trees([c.shape[1] for c in codewords], lambda r, i: codewords[r][:, i],
                                        lambda r, k: heaps[r][cc.SLOT * k:cc.SLOT * k + cc.SLOT], expansion, t, proof_stream)


@pytest.mark.parametrize("log_n,t", [(8, 2), (10, 4), (14, 8)])
def test_fri_transcript_from_trees_is_fri_prove(log_n, t):
    N, expansion = 1 << log_n, 4
    coeffs = oracle.felt_array(SEED + log_n, 0, 3 * (N // expansion)).reshape(3, -1)
    omega = oracle.primitive_nth_root(N)
    cw = oracle.xevaluate_soa(coeffs, oracle.GENERATOR, omega, N)
    ref = oracle.fri_prove(cw, oracle.GENERATOR, omega, expansion, t)
    out = _transcript(ref["codewords"], expansion, t)
    assert out["roots"] == ref["roots"] and out["alphas"] == ref["alphas"] and out["indices"] == ref["indices"]
    assert out["proof_stream"].serialize() == ref["proof_stream"].serialize()
    # the alphas alone fix the later codewords: fold by fold from round 0
    w, g = omega, oracle.GENERATOR
    for r, alpha in enumerate(out["alphas"]):
        assert (oracle.fri_fold(ref["codewords"][r], alpha, g, w) == ref["codewords"][r + 1]).all()
        w, g = oracle.mul(w, w), oracle.mul(g, g)


@pytest.mark.parametrize("tag", ["d16_t2", "d64_t8", "d1024_t4", "test_fri_valid", "test_fri_disturbed", "d16_t2_prepushed"])
def test_fri_transcript_from_trees_golden_streams(tag):
    rec = load_golden("fri.json")[tag]
    d = 1 << rec["log_degree"]
    if tag.startswith("test_fri"):
        coeffs = np.zeros((3, d), dtype=np.uint64)
        coeffs[0] = np.arange(d, dtype=np.uint64)
    else:
        coeffs = oracle.felt_array(SEED, 0, 3 * d).reshape(d, 3).T.copy()
    cw = oracle.xevaluate_soa(coeffs, rec["offset"], rec["omega"], rec["N"])
    for i in rec.get("disturb", []):
        cw[:, i] = 0
    assert hashlib.sha256(np.ascontiguousarray(cw, dtype="<u8").tobytes()).hexdigest() == rec["codeword_sha"]
    ps = oracle.ProofStreamOracle()
    if rec["num_prepushed"]:
        r = [hashlib.blake2b(bytes([i])).digest() for i in range(2)]
        e = [oracle.make_xfe([oracle.felt(SEED + 88, 3 * i + k) for k in range(3)]) for i in range(3)]
        for o in [r[0], (e[0], e[1], e[2]), [r[1]]]:
            ps.push(o)
    codewords, w, g = [cw], rec["omega"], rec["offset"]
    for alpha in rec["alphas"]:
        codewords.append(oracle.fri_fold(codewords[-1], alpha, g, w))
        w, g = oracle.mul(w, w), oracle.mul(g, g)
    assert len(codewords) == rec["rounds"]
    out = _transcript(codewords, rec["expansion"], rec["num_colinearity_tests"], ps)
    assert [x.hex() for x in out["roots"]] == rec["roots"] and out["alphas"] == rec["alphas"] and out["indices"] == rec["indices"]
    assert len(ps.objects) == rec["num_objects"]
    assert ps.serialize() == golden_bytes("fri_%s_stream.bin" % tag)


def mandatory_rows(n, workgroup):
    """what sample_rows must contain whatever the seed, spelt out once more for the test of sample_rows"""
    step = 1 << 20 if n > 1 << 20 else 1 << 16
    rows = [i for i in range(2 * workgroup)] + [n - 1 - i for i in range(2 * workgroup)]
    for c in [n // 2] + [q * (n // 4) for q in (1, 2, 3)] + [m * step for m in range(1, (n - 1) // step + 1)]:
        rows += [c + d for d in range(-workgroup, workgroup)]
    k = 1
    while k <= n:
        rows += [k - 2, k - 1, k, k + 1]
        k <<= 1
    return {r for r in rows if 0 <= r < n}


@pytest.mark.parametrize("n", [1 << 17, (1 << 20) + 5, 1 << 24])
@pytest.mark.parametrize("workgroup", [64, 256])
def test_sample_rows(n, workgroup):
    rows = cc.sample_rows(n, workgroup, seed=7, extra=(5, n - 7, n + 3, -1))
    assert rows == sorted(set(rows)) and rows[0] == 0 and rows[-1] == n - 1
    have = set(rows)
    assert mandatory_rows(n, workgroup) <= have and {5, n - 7} <= have
    # spelt out: both ends, the middle, the quarters, the 2^20 / 2^16 multiples, the powers of two
    step = 1 << 20 if n > 1 << 20 else 1 << 16
    for c in (n // 2, n // 4, 3 * (n // 4), step, (n - 1) // step * step):
        assert {c - workgroup, c - 1, c, min(c + workgroup, n) - 1} <= have
    assert set(range(2 * workgroup)) <= have and set(range(n - 2 * workgroup, n)) <= have
    assert all(r in have for k in range(1, 25) for r in range((1 << k) - 2, (1 << k) + 2) if r < n)
    assert len(have - mandatory_rows(n, workgroup) - {5, n - 7}) == 4096          # the uniform rows, on top of the others
    assert cc.sample_rows(n, workgroup, seed=7, extra=(5, n - 7, n + 3, -1)) == rows
    assert cc.sample_rows(n, workgroup, seed=8) != cc.sample_rows(n, workgroup, seed=7)


def test_sample_rows_of_tiny_trees():
    for n in (1, 2, 3, 65):
        assert cc.sample_rows(n, 64, seed=0) == list(range(n))
