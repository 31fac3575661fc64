"""A CPython model of FRI with one Merkle leaf per folding coset (Fri(..., folding_factor=a, coset_leaves=True), a = 2^k in (2, 4, 8)),
for tests/test_fri_coset_host.py and tests/test_gpu_fri_coset.py.  It has the shape of `fri_folding_model.prove` and is built only from
`oracle.fri_fold`, `oracle.MerkleOracle`, `oracle.dumps`, `oracle.make_xfe`, `oracle.ProofStreamOracle`, `oracle.sample_indices` and
`oracle.xsample` (the folds through fri_folding_model.fold_round, which adds `oracle.mul`).

Protocol.  L = log2(N / expansion), F = (L - 1) // k folds, codewords C_0 .. C_F, q_i = len(C_i) / a = len(C_{i+1}).
Commit: for i < F the tree of round i has q_i leaves, leaf c = blake2b(pickle.dumps((C_i[c], C_i[c + q_i], .., C_i[c + (a - 1) q_i]))) --
the tuple of distinct element objects, unsalted: the reference's Merkle over a list of tuples; the tree of C_F is one leaf per element.
Roots are pushed for r > 0, one challenge per round, the folds are fri_folding_model's; the last codeword's element objects are pushed as
a list.  Query: top-level indices sample_indices(seed, len(C_1), len(C_F), t); per layer i < F, with c_i = index mod q_i: first the t
tuples (C_i[c_i + j q_i]), j < a, then the t paths of leaf c_i in tree i (log2 q_i digests each).  Nothing of C_{i+1} is opened on
layer i: the value the tuple folds to is element number c_i // q_{i+1} of the tuple opened on layer i + 1 (or last_codeword[c_i]).
One Python object per (round, index); indices distinct mod len(C_F) are distinct mod every q_i, so no object recurs in the openings.
"""
import numpy as np

import fri_folding_model as folding

num_folds = folding.num_folds
fold_round = folding.fold_round
codeword_of = folding.codeword_of


def element_objects(o, cw):
    return [o.make_xfe([cw[0, i], cw[1, i], cw[2, i]]) for i in range(cw.shape[1])]


def coset_tuples(objs, a):
    """leaf c of the coset tree over a codeword's element objects: (objs[c], objs[c + q], .., objs[c + (a - 1) q])"""
    q = len(objs) // a
    return [tuple(objs[c + j * q] for j in range(a)) for c in range(q)]


def coset_merkle(o, cw, a):
    """-> (MerkleOracle over the pickles of the coset tuples, the tuples, the element objects)"""
    objs = element_objects(o, cw)
    tuples = coset_tuples(objs, a)
    return o.MerkleOracle([o.dumps(t) for t in tuples]), tuples, objs


def prove(o, cw_soa, offset, omega, expansion, t, folding_factor, proof_stream=None):
    """-> dict(indices, proof_stream, codewords, roots, alphas, rounds, trees)"""
    a = folding_factor
    k = a.bit_length() - 1
    assert a in (2, 4, 8)
    ps = proof_stream if proof_stream is not None else o.ProofStreamOracle()
    cw = np.ascontiguousarray(cw_soa, dtype=np.uint64)
    N = cw.shape[1]
    F = num_folds(N, expansion, k)
    assert F >= 1
    codewords, trees, leaves, roots, alphas = [], [], [], [], []
    w, g = omega, offset
    for r in range(F + 1):
        if r < F:
            tree, tuples, _ = coset_merkle(o, cw, a)
        else:
            tuples = element_objects(o, cw)                    # the last codeword: one leaf per element
            tree = o.MerkleOracle([o.dumps(e) for e in tuples])
        roots.append(tree.root())
        if r > 0:
            ps.push(tree.root())
        codewords.append(cw); trees.append(tree); leaves.append(tuples)
        if r == F:
            break
        alpha = o.xsample(ps.prover_fiat_shamir())
        alphas.append(alpha)
        cw, g, w = fold_round(o, cw, alpha, g, w, k)
    ps.push(leaves[F])
    top = o.sample_indices(ps.prover_fiat_shamir(), codewords[1].shape[1], codewords[F].shape[1], t)
    for i in range(F):
        q = codewords[i].shape[1] // a
        cs = [x % q for x in top]
        for s in range(t):
            ps.push(leaves[i][cs[s]])
        for s in range(t):
            ps.push(trees[i].open(cs[s]))
    return {"indices": top, "proof_stream": ps, "codewords": codewords, "roots": roots, "alphas": alphas, "rounds": F + 1, "trees": trees}


def count_digests(objects):
    """authentication-path digests among a stream's objects: the 64-byte items of its lists (the last codeword is a list of elements)"""
    return sum(1 for obj in objects if isinstance(obj, list) for item in obj if isinstance(item, (bytes, bytearray)) and len(item) == 64)


# ---- codewords for the stand-alone coset trees (tests/test_coset_emulation.py, tests/test_gpu_fri_coset.py) ----
P = (1 << 64) - (1 << 32) + 1
EDGE_ROWS = (0, 1, 62, 63, 64, 65, 127, 128, 255, 256)          # leaf rows at the edges of a wavefront (64 leaves = one workgroup)


def tree_codeword(o, seed, n, a, stride=None, planted=None):
    """(3, stride) words: n pseudo-random elements (junk behind them when stride > n).
    planted = "full": at the edge rows (and the last row) of the coset tree, elements whose limbs are one byte (0, 1, 255), two to five
    bytes and nine bytes (>= 2^63) long as pickle integers, the top limb never zero -- every tuple keeps three coefficients per element;
    planted = "short": there, elements that store 0, 1 and 2 coefficients as well, next to one- and nine-byte limbs."""
    stride = n if stride is None else stride
    cw = o.felt_array(seed, 0, 3 * stride).reshape(3, stride).copy()
    if planted is None:
        return cw
    q = n // a
    ints = [0, 1, 255, 256, 65535, 65536, (1 << 31) - 1, 1 << 31, (1 << 55) - 1, 1 << 55, (1 << 56) - 1, 1 << 56, (1 << 63) - 1, 1 << 63, P - 1]
    rows = sorted({r for r in EDGE_ROWS if r < q} | {q - 1})
    for x, row in enumerate(rows):
        for j in range(a):
            i = row + j * q
            pick = lambda y: ints[(3 * x + 5 * j + y) % len(ints)]
            limbs = [pick(0), pick(1), pick(2) or 1]
            if planted == "short":
                kept = (x + j) % 4                                  # 0 .. 3 coefficients
                limbs = [(v or 1) if y == kept - 1 else v for y, v in enumerate(limbs)]      # the top kept one is not zero
                limbs = [v if y < kept else 0 for y, v in enumerate(limbs)]
            cw[:, i] = limbs
    return cw


def tree_nodes(o, cw, n, a):
    """the reference's `nodes` of Merkle([coset tuples]) over the first n elements of cw, as MerkleOracle keeps them"""
    tree, _, _ = coset_merkle(o, np.ascontiguousarray(cw[:, :n]), a)
    return tree.nodes
