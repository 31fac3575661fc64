"""An independent check of the commitment layer: every parent of a Merkle tree, leaf digests at chosen rows, and the FRI transcript
assembled from trees that have been checked -- hashlib and CPython's pickle on the oracle's look-alike objects, nothing of the
product's native code.

A tree lies in memory the way the device keeps it: a heap of 64-byte slots, node k at byte 64 k, the root at k = 1, level L (the
root is level 0) at k in [2^L, 2^(L + 1)), the leaf digests at level `depth`.  The reference (merkle.py:26-41, restated by
oracle.MerkleOracle) fills its node list with 32 zero bytes and overwrites the slots of the leaves it has, so a parent above the
leaf level hashes 128, 96 or 64 bytes; the device never writes the absent slots, and nothing here reads them.

Two halves pin a tree: every parent is recomputed from its stored children (exhaustive at every size: ~1.2 us per parent), and the
leaf digests are recomputed from host copies of the committed data.  A leaf costs 30-50 us of pickle, so above ~2^17 leaves they
are sampled (sample_rows: the places where a leaf kernel's indexing can go wrong, plus uniform rows) together with the rows whose
data is unusual for the encoders (interesting_rows).

Every check returns a list of (kind, message) failures, as tests/pointwise_check.py does.  Used by tests/test_gpu_commitments_exact.py
on buffers read back from the GPU and by tests/test_commitment_checker.py on trees made with the oracle."""
from hashlib import blake2b

import numpy as np

from oracle import ref_oracle as oracle

SLOT = 64                       # bytes per node
_ABSENT = bytes(32)             # merkle.py:26 (32 zero bytes, not 64)
MAX_REPORTED = 20               # failures listed per call (the count of the rest is appended)


def tree_shape(n):
    """(next power of two, depth) of a tree of n leaves (merkle.py:9-20)"""
    npo2 = 1
    while npo2 < n:
        npo2 <<= 1
    return npo2, npo2.bit_length() - 1


def heap_reader(read_words):
    """read_level for a heap that read_words(count, offset) reads in 8-byte words (DeviceBuffer.to_numpy)"""
    def read_level(level, first, count):
        return read_words(8 * count, 8 * ((1 << level) + first)).tobytes()
    return read_level


def bytes_reader(heap):
    """read_level for a heap held in one bytes-like object"""
    view = memoryview(heap)

    def read_level(level, first, count):
        at = SLOT * ((1 << level) + first)
        return bytes(view[at:at + SLOT * count])
    return read_level


def _cut(failures, total):
    if total > len(failures):
        failures.append((failures[0][0], "... and %d more" % (total - len(failures))))
    return failures


def check_parents(read_level, depth, n_leaves, chunk=1 << 16):
    """every node k in [1, 2^depth) against blake2b(child 2k + child 2k+1).  read_level(level, first, count) returns the bytes of
    `count` nodes of `level` from the level's node `first` on; a level is read twice (as parents and as children), `chunk` parents
    at a time, so no more than 3 * chunk slots are on the host at once.  A leaf slot >= n_leaves counts as 32 zero bytes."""
    failures, total = [], 0
    for level in range(depth - 1, -1, -1):
        count = 1 << level
        for first in range(0, count, chunk):
            c = min(chunk, count - first)
            parents = read_level(level, first, c)
            present = 2 * c                                  # children of this chunk that exist
            if level + 1 == depth:
                present = max(0, min(2 * c, n_leaves - 2 * first))
            children = read_level(level + 1, 2 * first, present) if present else b""
            assert len(parents) == SLOT * c and len(children) == SLOT * present, "short read"
            whole = present // 2
            bad = [i for i in range(whole)
                   if blake2b(children[128 * i:128 * i + 128]).digest() != parents[SLOT * i:SLOT * i + SLOT]]
            for i in range(whole, c):                        # the ragged end of the level above the leaves
                left = children[128 * i:128 * i + SLOT] if 2 * i < present else _ABSENT
                if blake2b(left + _ABSENT).digest() != parents[SLOT * i:SLOT * i + SLOT]:
                    bad.append(i)
            total += len(bad)
            for i in bad[:max(0, MAX_REPORTED - len(failures))]:
                have = 2 if i < whole else (1 if 2 * i < present else 0)
                failures.append(("parent", "level %d index %d (heap %d, %d of 2 children present)" % (level, first + i, count + first + i, have)))
    return _cut(failures, total)


def sample_rows(n, workgroup, seed, extra=(), uniform=4096):
    """the leaves to recompute: the first and the last two workgroups, a workgroup either side of n/2, of every n/4 boundary and of
    every multiple of 2^20 (2^16 when n <= 2^20), two rows either side of every power of two, `extra`, and `uniform` uniform rows."""
    rows = set(range(min(n, 2 * workgroup))) | set(range(max(0, n - 2 * workgroup), n))
    step = 1 << 20 if n > 1 << 20 else 1 << 16
    centres = {n // 2, n // 4, 2 * (n // 4), 3 * (n // 4)} | set(range(step, n, step))
    for c in centres:
        rows.update(range(c - workgroup, c + workgroup))
    for k in range(n.bit_length() + 1):
        rows.update(range((1 << k) - 2, (1 << k) + 2))
    rows.update(int(i) for i in extra)
    rows = {r for r in rows if 0 <= r < n}
    rng, want = np.random.default_rng(seed), min(n, len(rows) + uniform)
    while len(rows) < want:                                  # `uniform` rows that are not in the set yet
        for i in rng.integers(0, n, uniform):
            if len(rows) < want:
                rows.add(int(i))
    return sorted(rows)


def check_leaves(read_digest, rows, preimage_of):
    """blake2b(preimage_of(i)) against the stored digest read_digest(i) for every i of rows"""
    failures, total = [], 0
    for i in rows:
        pre = preimage_of(i)
        if blake2b(pre).digest() != bytes(read_digest(i)):
            total += 1
            if len(failures) < MAX_REPORTED:
                failures.append(("leaf", "row %d (preimage of %d bytes)" % (i, len(pre))))
    return _cut(failures, total)


def digest_reader(leaf_level):
    """read_digest for a leaf level held as bytes / a uint64 array"""
    view = memoryview(leaf_level).cast("B") if not isinstance(leaf_level, (bytes, bytearray)) else memoryview(leaf_level)
    return lambda i: view[SLOT * i:SLOT * i + SLOT]


# ------------------------------------------------------------------ leaf preimages, from host copies of the committed data
def xfe_preimage(soa, i):
    """pickle of extension element i of a (3, n) codeword (merkle.py:30)"""
    return oracle.dumps(oracle.make_xfe([int(soa[0, i]), int(soa[1, i]), int(soa[2, i])]))


def bfe_preimage(values, i):
    return oracle.dumps(oracle.make_bfe(int(values[i])))


def row_preimage(columns, i, salt=None):
    """pickle of row i of the zipped `columns` -- a list of (3, n) arrays (extension columns) and (n,) arrays (base columns) in the
    order of the zip (brainfuck_stark.py:178-179) -- followed by the pickle of its salt (salted_merkle.py:32-35)"""
    row = tuple(oracle.make_xfe([int(c[0, i]), int(c[1, i]), int(c[2, i])]) if c.ndim == 2 else oracle.make_bfe(int(c[i])) for c in columns)
    return oracle.dumps(row) if salt is None else oracle.salted_leaf_bytes(row, salt)


class PickedRows:
    """the values of chosen rows of columns too large to keep: pick() copies a column's entries at `rows`; preimage(i, salt) is
    row_preimage on the copies"""

    def __init__(self, rows):
        self.rows = np.asarray(sorted(rows), dtype=np.int64)
        self._at = {int(r): j for j, r in enumerate(self.rows)}
        self.columns = []

    def pick(self, column):
        column = np.asarray(column)
        self.columns.append(np.ascontiguousarray(column[..., self.rows]))

    def preimage(self, i, salt=None):
        return row_preimage(self.columns, self._at[i], salt)


# ------------------------------------------------------------------ rows whose data is unusual for the leaf encoders
# pickle protocol 4 writes an int as BININT1 (< 2^8), BININT2 (< 2^16), BININT (< 2^31) or LONG1 with the fewest bytes of a signed
# little-endian number: 5 bytes below 2^39 (so [2^31, 2^32), which still fits 32 bits, is a class of its own), 6, 7, 8, then 9
WIDTH_CLASSES = [("int<2^8", 0, 1 << 8), ("int<2^16", 1 << 8, 1 << 16), ("int<2^31", 1 << 16, 1 << 31), ("int<2^32", 1 << 31, 1 << 32),
                 ("long5", 1 << 32, 1 << 39), ("long6", 1 << 39, 1 << 47), ("long7", 1 << 47, 1 << 55), ("long8", 1 << 55, 1 << 63),
                 ("long9", 1 << 63, 1 << 64)]


def width_class(v):
    return next(name for name, lo, hi in WIDTH_CLASSES if lo <= v < hi)


def stored_coefficients(soa):
    """per element of a (3, n) array: how many coefficients its stored polynomial has (trailing zero limbs dropped)"""
    soa = np.asarray(soa)
    return np.where(soa[2] != 0, 3, np.where(soa[1] != 0, 2, np.where(soa[0] != 0, 1, 0))).astype(np.int8)


def _widths(plane, found, cap, label):
    plane = np.asarray(plane, dtype=np.uint64)
    below = np.flatnonzero(plane < np.uint64(1 << 55))            # rare in a codeword: classified one by one class
    values = plane[below]
    for name, lo, hi in WIDTH_CLASSES[:7]:
        hit = below[(values >= np.uint64(lo)) & (values < np.uint64(hi))]
        if hit.size:
            found[(label, name)] = (int(hit.size), [int(i) for i in hit[:cap]])
    top = plane >= np.uint64(1 << 63)
    for name, mask in (("long9", top), ("long8", ~top & (plane >= np.uint64(1 << 55)))):
        hit = np.flatnonzero(mask)
        if hit.size:
            found[(label, name)] = (int(hit.size), [int(i) for i in hit[:cap]])


def interesting_rows(ext_columns=(), base_columns=(), cap=4, first=0):
    """{(column label, class): (rows found, the first `cap` of them)} over extension columns ((3, n) arrays: the stored-coefficient
    counts 0 ... 3 and the integer width of every limb) and base columns ((n,) arrays: the integer width); labels count from
    `first` so that one dictionary can be filled column by column"""
    found = {}
    for c, soa in enumerate(ext_columns):
        counts = stored_coefficients(soa)
        for k in range(4):
            hit = np.flatnonzero(counts == k)
            if hit.size:
                found[("x%d" % (first + c), "coefficients=%d" % k)] = (int(hit.size), [int(i) for i in hit[:cap]])
        for limb in range(3):
            _widths(soa[limb], found, cap, "x%d.%d" % (first + c, limb))
    for c, plane in enumerate(base_columns):
        _widths(plane, found, cap, "b%d" % (first + c))
    return found


def rows_of(found):
    return sorted({i for _, rows in found.values() for i in rows})


def class_counts(found):
    """{class: (rows found, rows checked)} summed over the columns, for printing"""
    out = {}
    for (_, name), (count, rows) in found.items():
        have = out.get(name, (0, 0))
        out[name] = (have[0] + count, have[1] + len(rows))
    return dict(sorted(out.items()))


def row_pattern(ext_columns, i):
    """the stored-coefficient counts of row i's extension elements: what selects a row's pickle template"""
    return tuple(int(stored_coefficients(c[:, i:i + 1])[0]) for c in ext_columns)


# ------------------------------------------------------------------ FRI transcript from checked trees
def fri_transcript_from_trees(lengths, element, node, expansion_factor, num_colinearity_tests, proof_stream=None):
    """oracle.fri_prove (fri.py:91-199) without pickling whole codewords: what the prover writes depends on the round roots, the
    last codeword and the opened elements and paths only.
      lengths      the lengths of the round codewords, N, N/2, ... (num_rounds of them)
      element(r, i)  the three limbs of element i of round r's codeword (a host copy)
      node(r, k)     the 64 bytes at heap index k of round r's tree, r < num_rounds - 1 (a tree that check_parents and
                     check_leaves have passed); the last round's tree is built here from the last codeword
    An element object is made once per (round, index) and a node once per (round, heap index): pickle memoises by identity, and
    the reference hands out the same list entries every time.  Returns roots, alphas, the top-level indices and the proof stream."""
    ps = proof_stream if proof_stream is not None else oracle.ProofStreamOracle()
    R, t = len(lengths), num_colinearity_tests
    assert R == oracle.fri_num_rounds(lengths[0], expansion_factor) and R >= 2, "one length per round"
    assert all(lengths[r] == lengths[0] >> r and lengths[r] & (lengths[r] - 1) == 0 for r in range(R)), "every round halves a power of two"
    elements, nodes = {}, {}

    def obj(r, i):
        if (r, i) not in elements:
            elements[(r, i)] = oracle.make_xfe([int(v) for v in element(r, i)])
        return elements[(r, i)]

    def path(r, index):
        out, k = [], lengths[r] | index
        while k > 1:
            if (r, k ^ 1) not in nodes:
                nodes[(r, k ^ 1)] = bytes(node(r, k ^ 1))
            out.append(nodes[(r, k ^ 1)])
            k >>= 1
        return out
    last_objs = [obj(R - 1, i) for i in range(lengths[-1])]
    last_tree = oracle.MerkleOracle([oracle.dumps(o) for o in last_objs])
    roots = [bytes(node(r, 1)) for r in range(R - 1)] + [last_tree.root()]
    alphas = []
    for r in range(R):                                        # fri.py:100-131
        if r > 0:
            ps.push(roots[r])
        if r == R - 1:
            break
        alphas.append(oracle.xsample(ps.prover_fiat_shamir()))
    ps.push(last_objs)                                        # fri.py:134
    top = oracle.sample_indices(ps.prover_fiat_shamir(), lengths[1], lengths[-1], t)      # fri.py:186-187
    indices = list(top)
    for r in range(R - 2):                                    # fri.py:191-194, query (141-158)
        half = lengths[r] // 2
        indices = [x % half for x in indices]
        for s in range(t):
            ps.push((obj(r, indices[s]), obj(r, indices[s] + half), obj(r + 1, indices[s])))
        for s in range(t):
            ps.push(path(r, indices[s])); ps.push(path(r, indices[s] + half)); ps.push(path(r + 1, indices[s]))
    indices = [x % lengths[-1] for x in indices]              # fri.py:195-197, query_last (160-176)
    half = lengths[-2] // 2
    for s in range(t):
        ps.push((obj(R - 2, indices[s]), obj(R - 2, indices[s] + half), last_objs[indices[s]]))
    for s in range(t):
        ps.push(path(R - 2, indices[s])); ps.push(path(R - 2, indices[s] + half))
    return {"roots": roots, "alphas": alphas, "indices": top, "proof_stream": ps, "rounds": R}
