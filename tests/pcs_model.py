"""A CPython model of the polynomial commitment (stark_brainfuck_amd/pcs.py: commit / open / verify) for tests/test_pcs_host.py and
tests/test_gpu_pcs.py: built on `oracle` (xmul, xinv, xsample, fast_coset_evaluate, ProofStreamOracle, MerkleOracle, dumps, make_xfe,
make_bfe) and on the three FRI models, unchanged.

Protocol.  m columns f_p over the domain x_i = offset * omega^i, i < N: extension polynomials first, then base polynomials.
  commit: leaf i of the row tree = blake2b(pickle.dumps((f_0(x_i), .., f_{m-1}(x_i)))), extension elements as `oracle.make_xfe` makes them,
          base elements pointing at the extension field's own BaseField instance (`make_bfe(v, internal=True)`); the root is pushed.
  open:   push the points (a list of elements), push the values (a list per point of a list per column, in row order);
          lambda = xsample(prover_fiat_shamir());
          g[i] = sum_j (lambda^(j m) S_i - Y_j) / (x_i - z_j),  S_i = sum_p lambda^p f_p(x_i),  Y_j = sum_p lambda^(j m + p) y_{p,j};
          push the root of Merkle(g) -- of the coset tree of g when the FRI mode commits to cosets;
          t indices int(blake2b(seed + bytes(s))) mod N, s < t, seed = prover_fiat_shamir()  (BrainfuckStark.sample_indices);
          per index i: the row tuple, its path, then the opening of g: the element g[i] and its path, or with coset leaves the tuple of
          leaf c = i mod (N / a) and its path.  One Python object per row, per element and per coset: an index drawn twice pushes the
          same objects twice;
          FRI over g on the same stream (fri_grinding_model.prove).  Per-element modes: where FRI opens, in round 0, an element whose
          object is already in the stream, it is that object (Fri.prove's known_leafs) -- the model hands the FRI model an `oracle`
          whose first xfe_merkle call returns those objects in their places; the tree of round 0 is FRI's own (fresh digest objects).
  verify: the same in reverse; the FRI layer itself is judged by the `fri_verify` the caller passes (the models have no FRI verifier).
`forced_values`: open with these values instead of the true ones, honest in everything else.
Bulk arithmetic runs on Python integers (xmul / xinv below, the same formulas; tests/test_pcs_host.py compares them with the oracle's).
"""
import hashlib

import numpy as np

import fri_coset_model
import fri_grinding_model

P = (1 << 64) - (1 << 32) + 1


# ---- F_p[X]/(X^3 - X + 1) on Python integers
def xadd(a, b): return ((a[0] + b[0]) % P, (a[1] + b[1]) % P, (a[2] + b[2]) % P)
def xsub(a, b): return ((a[0] - b[0]) % P, (a[1] - b[1]) % P, (a[2] - b[2]) % P)


def xmul(a, b):
    d0 = a[0] * b[0]
    d1 = a[0] * b[1] + a[1] * b[0]
    d2 = a[0] * b[2] + a[1] * b[1] + a[2] * b[0]
    d3 = a[1] * b[2] + a[2] * b[1]
    d4 = a[2] * b[2]
    return ((d0 - d3) % P, (d1 + d3 - d4) % P, (d2 + d4) % P)          # X^3 = X - 1, X^4 = X^2 - X


def xinv(a):
    """by the adjugate of the matrix of multiplication by a; its determinant is the norm"""
    a0, a1, a2 = a
    s, d = (a0 + a2) % P, (a1 - a2) % P
    c0, c1, c2 = (s * s - d * a1) % P, (d * a2 - a1 * s) % P, (a1 * a1 - s * a2) % P
    norm = (a0 * c0 - a2 * c1 - a1 * c2) % P
    ninv = pow(norm, P - 2, P)
    return (c0 * ninv % P, c1 * ninv % P, c2 * ninv % P)


def xpow(a, e):
    acc = (1, 0, 0)
    while e:
        if e & 1:
            acc = xmul(acc, a)
        a, e = xmul(a, a), e >> 1
    return acc


# ---- the two kernels' arithmetic
def evaluate_base(column, z):
    """sum_i column[i] z^i by Horner's rule"""
    acc = (0, 0, 0)
    for c in reversed([int(v) for v in column]):
        acc = xmul(acc, z)
        acc = ((acc[0] + c) % P, acc[1], acc[2])
    return acc


def evaluate_ext(soa, z):
    """an extension polynomial with limb planes soa[0..3): v0 + X v1 + X^2 v2 of the planes' values"""
    v = [evaluate_base(soa[k], z) for k in range(3)]
    X = (0, 1, 0)
    return xadd(v[0], xadd(xmul(v[1], X), xmul(v[2], xmul(X, X))))


def combined_values(values, lam):
    """Y_j = sum_p lambda^(j m + p) y_{p,j}"""
    out, power = [], (1, 0, 0)
    for per_point in values:
        acc = (0, 0, 0)
        for y in per_point:
            acc = xadd(acc, xmul(power, tuple(y)))
            power = xmul(power, lam)
        out.append(acc)
    return out


def quotient(columns, N, offset, omega, points, Y, lam):
    """columns: per column a 1-D array of N words (base) or a (3, >= N) array (extension) -> g as a (3, N) array"""
    m, k = len(columns), len(points)
    powers = [(1, 0, 0)]
    for _ in range(k * m):
        powers.append(xmul(powers[-1], lam))
    cols = [(np.asarray(c).ndim == 2, [[int(v) for v in plane[:N]] for plane in c] if np.asarray(c).ndim == 2 else [int(v) for v in c[:N]]) for c in columns]
    out = np.zeros((3, N), dtype=np.uint64)
    x = offset % P
    for i in range(N):
        s = (0, 0, 0)
        for p, (is_ext, data) in enumerate(cols):
            w = powers[p]
            if is_ext:
                s = xadd(s, xmul(w, (data[0][i], data[1][i], data[2][i])))
            else:
                v = data[i]
                s = ((s[0] + w[0] * v) % P, (s[1] + w[1] * v) % P, (s[2] + w[2] * v) % P)
        g = (0, 0, 0)
        for j in range(k):
            num = xsub(xmul(powers[j * m], s), Y[j])
            g = xadd(g, xmul(num, xinv(xsub((x, 0, 0), points[j]))))
        out[0, i], out[1, i], out[2, i] = g
        x = x * omega % P
    return out


def in_domain(z, N, offset):
    return z[1] == 0 and z[2] == 0 and pow(z[0] * pow(offset, P - 2, P) % P, N, P) == 1


def sample_indices(t, seed, N):
    return [int.from_bytes(hashlib.blake2b(seed + bytes(s)).digest(), "big") % N for s in range(t)]


# ---- commit / open / verify
def commit(o, ext_polys, base_polys, N, offset, omega, proof_stream=None):
    """ext_polys: (3, d) coefficient arrays; base_polys: 1-D coefficient arrays -> dict(codewords, rows, tree, proof_stream); pushes the root"""
    ps = proof_stream if proof_stream is not None else o.ProofStreamOracle()
    codewords = [o.xevaluate_soa(np.asarray(f, dtype=np.uint64), offset, omega, N) for f in ext_polys]
    codewords += [o.fast_coset_evaluate(np.asarray(f, dtype=np.uint64), offset, omega, N) for f in base_polys]
    n_ext = len(ext_polys)

    def row(i):
        return tuple([o.make_xfe([c[0, i], c[1, i], c[2, i]]) for c in codewords[:n_ext]] + [o.make_bfe(c[i], internal=True) for c in codewords[n_ext:]])
    rows = [row(i) for i in range(N)]
    tree = o.MerkleOracle([o.dumps(r) for r in rows])
    ps.push(tree.root())
    return {"ext": [np.asarray(f, dtype=np.uint64) for f in ext_polys], "base": [np.asarray(f, dtype=np.uint64) for f in base_polys],
            "codewords": codewords, "rows": rows, "tree": tree, "root": tree.root(), "proof_stream": ps, "N": N}


def true_values(committed, points):
    return [[evaluate_ext(f, z) for f in committed["ext"]] + [evaluate_base(f, z) for f in committed["base"]] for z in points]


class _KnownLeafs:
    """`oracle` for the FRI model of a per-element mode: the first xfe_merkle call (round 0, over g) gets the element objects that are in
    the stream already in their places; everything else is the oracle's"""

    def __init__(self, o, known):
        self._o, self._known = o, dict(known)

    def __getattr__(self, name):
        return getattr(self._o, name)

    def xfe_merkle(self, cw):
        tree, objs = self._o.xfe_merkle(cw)
        known, self._known = self._known, {}
        for i, e in known.items():
            assert self._o.xfe_limbs(e) == [int(cw[0, i]), int(cw[1, i]), int(cw[2, i])]
            objs[i] = e
        return tree, objs


def open(o, committed, points, offset, omega, expansion, t, folding_factor=2, coset_leaves=False, grinding_bits=0, forced_values=None):
    """-> dict(values, lam, g, g_root, indices, fri, proof_stream, bytes); points: limb triples outside the domain"""
    ps, N = committed["proof_stream"], committed["N"]
    points = [tuple(int(v) for v in z) for z in points]
    assert 1 <= len(points) <= 4 and not any(in_domain(z, N, offset) for z in points)
    ps.push([o.make_xfe(z) for z in points])
    values = true_values(committed, points) if forced_values is None else [[tuple(int(x) for x in v) for v in per] for per in forced_values]
    ps.push([[o.make_xfe(v) for v in per_point] for per_point in values])
    lam = tuple(int(v) for v in o.xsample(ps.prover_fiat_shamir()))
    g = quotient(committed["codewords"], N, offset, omega, points, combined_values(values, lam), lam)
    a = folding_factor if coset_leaves else 1
    q = N // a
    if coset_leaves:
        tree, leaves, _ = fri_coset_model.coset_merkle(o, g, a)
    else:
        tree, leaves = o.xfe_merkle(g)
    ps.push(tree.root())
    indices = sample_indices(t, ps.prover_fiat_shamir(), N)
    for i in indices:
        ps.push(committed["rows"][i])
        ps.push(committed["tree"].open(i))
        ps.push(leaves[i % q])
        ps.push(tree.open(i % q))
    oo = o if coset_leaves else _KnownLeafs(o, {i: leaves[i] for i in indices})
    fri = fri_grinding_model.prove(oo, g, offset, omega, expansion, t, folding_factor, coset_leaves, grinding_bits, proof_stream=ps)
    out = fri["proof_stream"]
    return {"values": values, "lam": lam, "g": g, "g_root": tree.root(), "indices": indices, "fri": fri, "proof_stream": out,
            "bytes": out.serialize(), "points": points}


def verify(o, objects, root, points, values, N, offset, omega, t, folding_factor, coset_leaves, fri_verify):
    """objects: the stream's objects (the oracle's classes) from the commitment's root on (objects[0] is that root).
    fri_verify(objects, read_index, g_root) -> bool judges what lies behind the openings.  -> (verdict, reason)"""
    ps = o.ProofStreamOracle()
    ps.objects = list(objects)
    at = [1]

    def pull():
        at[0] += 1
        return ps.objects[at[0] - 1]

    def fiat_shamir():
        prefix = o.ProofStreamOracle()
        prefix.objects = ps.objects[:at[0]]
        return prefix.prover_fiat_shamir()
    points = [tuple(int(v) for v in z) for z in points]
    values = [[tuple(int(x) for x in v) for v in per] for per in values]
    if objects[0] != root:
        return False, "root"
    if any(in_domain(z, N, offset) for z in points):
        return False, "points"
    if [tuple(o.xfe_limbs(z)) for z in pull()] != points:
        return False, "points"
    if [[tuple(o.xfe_limbs(v)) for v in per] for per in pull()] != values:
        return False, "values"
    lam = tuple(int(v) for v in o.xsample(fiat_shamir()))
    Y = combined_values(values, lam)
    g_root = pull()
    indices = sample_indices(t, fiat_shamir(), N)
    a = folding_factor if coset_leaves else 1
    q = N // a
    m = len(values[0])
    for i in indices:
        row, path = pull(), pull()
        if not o.merkle_verify(root, i, path, o.dumps(row)):
            return False, "row path"
        leaf, path = pull(), pull()
        if not o.merkle_verify(g_root, i % q, path, o.dumps(leaf)):
            return False, "quotient path"
        columns = [np.array(o.xfe_limbs(e), dtype=np.uint64).reshape(3, 1) if hasattr(e, "polynomial") else np.array([e.value], dtype=np.uint64) for e in row]
        if len(columns) != m:
            return False, "row"
        x = offset * pow(omega, i, P) % P
        want = quotient(columns, 1, x, 1, points, Y, lam)
        if [int(v) for v in want[:, 0]] != [int(v) for v in o.xfe_limbs(leaf[i // q] if coset_leaves else leaf)]:
            return False, "quotient value"
    return (True, "accepted") if fri_verify(ps.objects, at[0], g_root) else (False, "fri")
