"""Exact checkers for the subproduct tree (csrc/subproduct.hip) that look at EVERY output and never call the product's code.

The three operations have unique answers, so evaluating on the oracle decides them completely:
  * evaluate: the values of the given coefficients at the n points;
  * interpolate: the one vector of exactly n words whose polynomial takes the given values at the n (distinct) points;
  * zerofier: the one vector of n + 1 words with word n = 1 whose polynomial vanishes at the n (distinct) points.
No O(n^2) work is needed when the points are ones the oracle's coset transform reaches: a domain is built from points c * w_M^j of
cosets c <w_M> of power-of-two subgroups, a seeded subset in seeded order, plus a handful of FREE points (0, 1, p - 1, ...) that
are evaluated by Horner's rule on Python integers.  oracle.fast_coset_evaluate(coeffs, c, w_E, E) with E >= max(M, len(coeffs))
gives the polynomial on c <w_E>, every (E / M)-th output is a point of c <w_M>.

A Domain is a list of groups ("coset", c, M, exponents) and ("free", x) and a placement: the points of the groups, concatenated in
group order, go to positions placement[0], placement[1], ... of the domain.

The last part restates node_deg and the case analysis of ptree_evaluate in Python, for coverage accounting only: which node shapes and
which quotient lengths the sizes below reach (tests/test_subproduct_checker.py holds the floor).  No expected value comes from it."""
import itertools
import random

import numpy as np

import field_states
from oracle import ref_oracle as oracle

P = (1 << 64) - (1 << 32) + 1
OFFSETS = (7, pow(7, 3, P), pow(7, 5, P), pow(7, 11, P))       # distinct cosets of every power-of-two subgroup, none holds 0, 1 or p - 1
FREE_POINTS = (0, 1, P - 1, 2, (1 << 32) - 1, 1 << 32, P - (1 << 32))
LEAF_LOG = 7                                                   # PT_LEAF_LOG: a subtree of 128 leaves is one workgroup


def log2_ceil(x):
    return max(int(x) - 1, 0).bit_length()


# ------------------------------------------------------------------------------------------------ domains
class Domain:
    """entries: one ("coset", c, M, e) (the point c * w_M^e) or ("free", x) per position of the domain"""

    def __init__(self, entries, order=None):
        self.entries = [tuple(e) for e in entries]
        self.n = len(self.entries)
        self.order = order                  # table_shape: the root order the reference would be called with
        cosets, free = {}, []
        for pos, e in enumerate(self.entries):
            if e[0] == "coset":
                _, c, M, k = e
                assert M >= 1 and M & (M - 1) == 0 and 0 <= k < M and 0 < c < P
                cosets.setdefault((c, M), []).append((pos, k))
            else:
                assert e[0] == "free" and 0 <= e[1] < P
                free.append((pos, e[1]))
        self.groups, placement = [], []
        for (c, M), members in cosets.items():
            self.groups.append(("coset", c, M, np.array([k for _, k in members], dtype=np.int64)))
            placement += [pos for pos, _ in members]
        for pos, x in free:
            self.groups.append(("free", x))
            placement.append(pos)
        self.placement = np.array(placement, dtype=np.int64)
        assert sorted(placement) == list(range(self.n))

    def __len__(self):
        return self.n

    def scatter(self, per_group):
        """per-group results (an array per coset group, one word per free group), concatenated, into domain order"""
        flat = np.concatenate([np.atleast_1d(np.asarray(g, dtype=np.uint64)) for g in per_group]) if per_group else np.zeros(0, dtype=np.uint64)
        out = np.empty(self.n, dtype=np.uint64)
        out[self.placement] = flat
        return out


def _root(order):
    return oracle.primitive_nth_root(order) if order > 1 else 1


def _coset_points(c, M):
    """c * w_M^j, j < M: the oracle's coset evaluation of the polynomial X"""
    if M == 1:
        return np.array([c], dtype=np.uint64)
    return oracle.fast_coset_evaluate(np.array([0, 1], dtype=np.uint64), c, _root(M), M)


def points(domain):
    """the domain as a uint64 array"""
    return domain.scatter([_coset_points(g[1], g[2])[g[3]] if g[0] == "coset" else g[1] for g in domain.groups])


def free_positions(n, count):
    """where `count` free points go: first, last, and on both sides of the subtree boundaries (127 | 128 and the last multiple of 128)"""
    last = ((n - 1) >> LEAF_LOG) << LEAF_LOG
    wanted = [0, n - 1, 127, 128, last - 1, last, last + 1, 129, 126, 1, n - 2, 2, n - 3, 125, 130, 3]
    out = []
    for p in wanted:
        if 0 <= p < n and p not in out:
            out.append(p)
    assert len(out) >= count, "no room for %d free points among %d" % (count, n)
    return out[:count]


def ragged(n, seed, free=()):
    """n distinct points: a seeded subset, in seeded order, of the four cosets OFFSETS[k] <w_M>, M = 2^ceil(log2 n) (at least 2),
    with the free points at free_positions"""
    M = max(1 << log2_ceil(n), 2)
    rng = random.Random((seed << 20) ^ n)
    where = dict(zip(free_positions(n, len(free)), free))
    picks = rng.sample(range(4 * M), n - len(free))
    entries, k = [], 0
    for pos in range(n):
        if pos in where:
            entries.append(("free", where[pos]))
        else:
            entries.append(("coset", OFFSETS[picks[k] // M], M, picks[k] % M))
            k += 1
    dom = Domain(entries)
    assert len(set(points(dom).tolist())) == n
    return dom


def table_shape(k, r, order=None):
    """what Table.interpolate_columns passes for a 2^k-row table with r randomizers: omicron^i, i < 2^k, in order, then the first r
    odd powers of w_order -- the coset 1 <w_(2^k)> and r points of the coset w_order <w_order^2>"""
    order = (1 << (k + 3)) if order is None else order
    assert order >= (2 << k) and r <= order // 2
    entries = [("coset", 1, 1 << k, i) for i in range(1 << k)] + [("coset", _root(order), order // 2, i) for i in range(r)]
    return Domain(entries, order=order)


def with_equal(domain, pairs):
    """the domain with position b holding the point of position a, for every (a, b) of pairs"""
    entries = list(domain.entries)
    for a, b in pairs:
        entries[b] = entries[a]
    return Domain(entries, order=domain.order)


# ------------------------------------------------------------------------------------------------ the reference and the checkers
def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % P
    return acc


def evaluate_everywhere(domain, coeffs):
    """the polynomial with these coefficients at every point of the domain, in domain order: one oracle transform per coset group,
    Horner on Python integers for the free points"""
    coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1)
    assert (coeffs < np.uint64(P)).all(), "a coefficient is no canonical residue"
    ints = None
    per_group = []
    for g in domain.groups:
        if g[0] == "free":
            ints = [int(v) for v in coeffs] if ints is None else ints
            per_group.append(horner(ints, g[1]))
            continue
        _, c, M, exps = g
        if coeffs.size == 0:
            per_group.append(np.zeros(exps.size, dtype=np.uint64))
            continue
        E = max(M, 1 << log2_ceil(coeffs.size))
        if E == 1:                                   # one coefficient on a one-point group
            per_group.append(np.full(exps.size, coeffs[0], dtype=np.uint64))
            continue
        wE = _root(E)
        assert M == 1 or oracle.power(wE, E // M) == _root(M)
        per_group.append(oracle.fast_coset_evaluate(coeffs, c, wE, E)[exps * (E // M)])
    return domain.scatter(per_group)


def _first_difference(got, want):
    bad = np.flatnonzero(got != want)
    return int(bad[0]) if bad.size else None


def _words(got, length, what):
    got = np.asarray(got)
    assert got.ndim == 1 and got.size == length, "%s: %s words, expected %d" % (what, got.shape, length)
    got = got.astype(np.uint64)
    k = _first_difference(got < np.uint64(P), True)
    assert k is None, "%s: word %d is 0x%X, no canonical residue" % (what, k, int(got[k]))
    return got


def check_evaluate(domain, coeffs, got):
    got = _words(got, len(domain), "evaluation")
    want = evaluate_everywhere(domain, coeffs)
    k = _first_difference(got, want)
    assert k is None, "evaluation of %d coefficients: position %d of %d is %d, expected %d (%d positions differ)" % (
        np.asarray(coeffs).size, k, len(domain), int(got[k]), int(want[k]), int((got != want).sum()))


def check_interpolant(domain, values, got):
    n = len(domain)
    got = _words(got, n, "interpolant")
    values = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1)
    assert values.size == n
    at = evaluate_everywhere(domain, got)
    k = _first_difference(at, values)
    assert k is None, "interpolant over %d points: at position %d it takes %d, not %d (%d positions differ)" % (
        n, k, int(at[k]), int(values[k]), int((at != values).sum()))


def check_zerofier(domain, got):
    n = len(domain)
    got = _words(got, n + 1, "zerofier")
    assert int(got[n]) == 1, "zerofier of %d points: word %d is %d, not 1" % (n, n, int(got[n]))
    at = evaluate_everywhere(domain, got)
    k = _first_difference(at, 0)
    assert k is None, "zerofier of %d points: %d at position %d (%d positions are no roots)" % (n, int(at[k]), k, int((at != 0).sum()))


def check_double_roots(domain, zerofier, positions):
    """a zerofier over a domain with repeated points: its derivative vanishes at the repeated ones too (Python integers)"""
    z = [int(v) for v in zerofier]
    dz = [(i * z[i]) % P for i in range(1, len(z))]
    pts = points(domain)
    for pos in positions:
        assert horner(dz, int(pts[pos])) == 0, "the point at position %d is no double root" % pos


# ------------------------------------------------------------------------------------------------ column kinds
KINDS = ("random", "zero", "pm1", "first", "last", "palette")
BATCH_KINDS = {1: ("random",), 3: ("random", "palette", "pm1"), 7: KINDS + ("random",)}


def column(kind, length, seed):
    """`length` words of coefficients or values"""
    out = np.zeros(length, dtype=np.uint64)
    if length == 0:
        return out
    if kind == "random":
        return oracle.felt_array(seed, 0, length)
    if kind == "pm1":
        out[:] = P - 1
    elif kind == "first":
        out[0] = oracle.felt(seed, 0) or 1
    elif kind == "last":
        out[-1] = oracle.felt(seed, 1) or 1
    elif kind == "palette":
        out[:] = [v for v, _ in zip(itertools.cycle(field_states.PALETTE), range(length))]
    else:
        assert kind == "zero"
    return out


def columns(batch, length, seed):
    """one column per kind of BATCH_KINDS[batch], the random ones from different seeds"""
    return np.stack([column(kind, length, seed + 977 * b) for b, kind in enumerate(BATCH_KINDS[batch])])


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
TREE_SIZES = (129, 255, 256, 257, 383, 384, 385, 640, 1000, 1023, 1025, 2052, 4095, 4100, 5000, 8193, 12289, (1 << 15) + 1)
FREE_SIZES = (257, 385, 4100, 8193)                  # these get FREE_POINTS
SMALL_SIZES = (1, 2, 3, 5)                           # one subtree, long polynomials: the l1 > l2 cases
LONG_LIMIT = 4100                                    # 2n + 5, 4n + 1, 8n + 3 coefficients up to this n


def coefficient_counts(n):
    """the coefficient counts m evaluated on a tree of n points"""
    if n in SMALL_SIZES:
        return sorted({n + 1, n + 129, 1000})
    N = 1 << log2_ceil(n)
    ms = {1, 2, n - 1, n, n + 1, n + 2, n + 128, n + 129}
    if N > n:
        ms |= {N, N + 1}
    if n <= LONG_LIMIT:
        ms |= {2 * n + 5, 4 * n + 1, 8 * n + 3}
    return sorted(m for m in ms if m >= 1)


def long_cases():
    """every (n, m) with m > n that the GPU tests evaluate"""
    return [(n, m) for n in SMALL_SIZES + TREE_SIZES for m in coefficient_counts(n) if m > n]


# ------------------------------------------------------------------------------------------------ coverage restatement (no values)
def node_deg(n, k, c):
    lo = c << k
    if lo >= n:
        return 0
    return min(n - lo, 1 << k)


def _node_class(d, k):
    return "full" if d == 1 << k else ("partial" if d else "empty")


def _ql_class(ql, k):
    return "0" if ql == 0 else ("1" if ql == 1 else ("2^k" if ql == 1 << k else "other"))


def shape_classes(n):
    """what the children of the levels above the LDS subtrees look like in a tree of n points: ("node", side, full | partial | empty)
    and, for the remainder tree (rem_quot_kernel), ("ql", side, 0 | 1 | 2^k | other) with ql = d_parent - d_child, 0 for an empty
    child.  side: "left" for an even node, "right" for an odd one."""
    L = log2_ceil(n)
    T = min(L, LEAF_LOG)
    out = set()
    for k in range(T, L):
        for c in range(1 << (L - k)):
            side = "right" if c & 1 else "left"
            d, dp = node_deg(n, k, c), node_deg(n, k + 1, c >> 1)
            out.add(("node", side, _node_class(d, k)))
            out.add(("ql", side, _ql_class(dp - d if d else 0, k)))
    return out


SHAPE_EXCLUDED = {
    ("ql", "right", "1"): "a right child with a point has a full left sibling: ql = 2^k >= 128",
    ("ql", "right", "other"): "a right child with a point has a full left sibling: ql = 2^k exactly",
}
SHAPE_REQUIRED = frozenset(
    [("node", side, cls) for side in ("left", "right") for cls in ("full", "partial", "empty")] +
    [("ql", side, q) for side in ("left", "right") for q in ("0", "1", "2^k", "other")]) - frozenset(SHAPE_EXCLUDED)


def long_classes(n, m):
    """the branch of ptree_evaluate for m > n coefficients, names as there: (class of ql = m - n: "1", "pow2", "pow2+1" or "other";
    "s2<=N" or "s2>N": the quotient is staged in R1 or in a block of its own; "l1>l2" or "l1<=l2": which transform is the larger)"""
    assert m > n >= 1
    N = 1 << log2_ceil(n)
    ql = m - n
    prec = 1 << log2_ceil(ql)
    l1, l2 = log2_ceil(2 * prec), log2_ceil(m)
    if ql == 1:
        q = "1"
    elif ql & (ql - 1) == 0:
        q = "pow2"
    elif (ql - 1) & (ql - 2) == 0:
        q = "pow2+1"
    else:
        q = "other"
    return (q, "s2>N" if (1 << l2) > N else "s2<=N", "l1>l2" if l1 > l2 else "l1<=l2")


def _long_excluded(state):
    q, s, l = state
    if l == "l1>l2" and q in ("1", "pow2"):
        return "l1 > l2 needs prec >= 2^l2 >= m = n + ql, and prec = ql when ql is a power of two"
    if l == "l1>l2" and s == "s2<=N":
        return "l1 > l2 needs prec >= m, so ql > prec / 2 >= m / 2: then m > 2n > N, and s2 >= m"
    return None


_LONG_STATES = list(itertools.product(("1", "pow2", "pow2+1", "other"), ("s2<=N", "s2>N"), ("l1>l2", "l1<=l2")))
LONG_EXCLUDED = {s: _long_excluded(s) for s in _LONG_STATES if _long_excluded(s)}
LONG_REQUIRED = frozenset(_LONG_STATES) - frozenset(LONG_EXCLUDED)
