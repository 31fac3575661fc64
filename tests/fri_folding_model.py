"""A CPython model of FRI with a folding factor a = 2^k in (2, 4, 8), for tests/test_fri_folding_host.py and
tests/test_gpu_fri_folding.py.  It has the shape of `oracle.fri_prove` and is built only from `oracle.fri_fold`,
`oracle.xfe_merkle`, `oracle.ProofStreamOracle`, `oracle.sample_indices`, `oracle.xsample` and `oracle.mul`.

Protocol.  L = log2(N / expansion), F = (L - 1) // k folds, codewords C_0 .. C_F with len(C_{r+1}) = len(C_r) / a.
Commit: per round the tree over C_r, its root pushed for r > 0; then (r < F) ONE challenge alpha_r, and C_{r+1} is k successive
reference folds of C_r with the challenges alpha_r^(2^j), offset and omega squared after each.  The last codeword's element objects
are pushed as a list.  Query: top-level indices sample_indices(seed, len(C_1), len(C_F), t); per layer i < F, with q = len(C_i) / a
and c = index mod q: first t tuples (C_i[c], C_i[c + q], .., C_i[c + (a - 1) q], C_{i+1}[c]), then per test the a paths of tree i
in that order and (except on the last layer) the path of c in tree i + 1.  One Python object per (round, index).
For a = 2 this is `oracle.fri_prove`'s stream byte for byte.
"""
import numpy as np


def num_folds(N, expansion, k):
    halvings = 0
    while N > expansion:
        N //= 2
        halvings += 1
    return (halvings - 1) // k


def _xsquare_from_mul(o, alpha):
    """alpha * alpha in F_p[X]/(X^3 - X + 1) from oracle.mul alone (schoolbook, X^3 = X - 1, X^4 = X^2 - X)"""
    P = (1 << 64) - (1 << 32) + 1
    a0, a1, a2 = (int(x) for x in alpha)
    m = o.mul
    d0, d1, d2, d3, d4 = m(a0, a0), 2 * m(a0, a1) % P, (2 * m(a0, a2) + m(a1, a1)) % P, 2 * m(a1, a2) % P, m(a2, a2)
    return [(d0 - d3) % P, (d1 + d3 - d4) % P, (d2 + d4) % P]


def fold_round(o, cw, alpha, offset, omega, k):
    """one round of the model: C_{r+1} from C_r, plus the offset and generator of the next round"""
    alpha = [int(x) for x in alpha]
    for _ in range(k):
        cw = o.fri_fold(cw, alpha, offset, omega)
        alpha, offset, omega = _xsquare_from_mul(o, alpha), o.mul(offset, offset), o.mul(omega, omega)
    return cw, offset, omega


def prove(o, cw_soa, offset, omega, expansion, t, folding_factor, proof_stream=None):
    """-> dict(indices, proof_stream, codewords, roots, alphas, rounds)"""
    a = folding_factor
    k = a.bit_length() - 1
    assert a in (2, 4, 8)
    ps = proof_stream if proof_stream is not None else o.ProofStreamOracle()
    cw = np.ascontiguousarray(cw_soa, dtype=np.uint64)
    N = cw.shape[1]
    F = num_folds(N, expansion, k)
    assert F >= 1
    codewords, trees, leaf_objs, roots, alphas = [], [], [], [], []
    w, g = omega, offset
    for r in range(F + 1):
        tree, objs = o.xfe_merkle(cw)
        roots.append(tree.root())
        if r > 0:
            ps.push(tree.root())
        codewords.append(cw); trees.append(tree); leaf_objs.append(objs)
        if r == F:
            break
        alpha = o.xsample(ps.prover_fiat_shamir())
        alphas.append(alpha)
        cw, g, w = fold_round(o, cw, alpha, g, w, k)
    ps.push(leaf_objs[F])
    top = o.sample_indices(ps.prover_fiat_shamir(), codewords[1].shape[1], codewords[F].shape[1], t)
    for i in range(F):
        q = codewords[i].shape[1] // a
        cs = [x % q for x in top]
        for s in range(t):
            ps.push(tuple(leaf_objs[i][cs[s] + j * q] for j in range(a)) + (leaf_objs[i + 1][cs[s]],))
        for s in range(t):
            for j in range(a):
                ps.push(trees[i].open(cs[s] + j * q))
            if i + 1 < F:
                ps.push(trees[i + 1].open(cs[s]))
    return {"indices": top, "proof_stream": ps, "codewords": codewords, "roots": roots, "alphas": alphas, "rounds": F + 1}


def codeword_of(o, seed, N, expansion, offset, omega, extra_degree=0):
    """the evaluations over offset * <omega> of a polynomial with N / expansion (+ extra_degree) pseudo-random extension coefficients,
    as an SoA (3, N) array; the coefficients include 0 and p - 1"""
    P = (1 << 64) - (1 << 32) + 1
    d = N // expansion + extra_degree
    coeffs = o.felt_array(seed, 0, 3 * d).reshape(3, d).copy()
    coeffs[0, 0], coeffs[1, d - 1] = 0, P - 1
    return o.xevaluate_soa(coeffs, offset, omega, N)
