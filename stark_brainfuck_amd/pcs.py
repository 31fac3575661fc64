"""A polynomial commitment from FRI: commit to polynomials, then prove what they evaluate to at points OUTSIDE the FRI domain.

    evaluate_at(coeffs, points)                       values of coefficient arrays in HBM at points of the extension field
    PolynomialCommitment(fri, hiding=False)
      .commit(polys, proof_stream) -> Commitment      codewords + one row tree in HBM (unsalted; salted with hiding=True); pushes the root
      .open(commitment, points, proof_stream)         pushes the opening proof; returns the values
      .verify(root, points, values, proof_stream)     host only (ints, hashlib, Fri.verify)

The reference has nothing of the kind: its STARK only ever opens committed codewords ON the domain.  The statement "the polynomial behind
this root takes the value y at z" is reduced to a low-degree test of the DEEP quotient (csrc/deep.hip, include/bfstark_ext.h)

    g(x) = sum_{j < k} ( lambda^(j m) * S(x) - Y_j ) / (x - z_j),   S = sum_{p < m} lambda^p f_p,   Y_j = sum_{p < m} lambda^(j m + p) y_{p,j}

over the m committed columns f_p (extension columns first, then base columns, each group in the caller's order) with one Fiat-Shamir
challenge lambda: g is a polynomial of degree < d exactly when every y_{p,j} = f_p(z_j).

Proof stream of `open`, after the root that `commit` pushed:
    the points (a list of elements); the values (a list per point of a list per polynomial, in row order);
    [lambda = xfield.sample(fiat_shamir)];  the root of the tree over g (Merkle, or CosetMerkle when the Fri commits to cosets);
    [t indices = BrainfuckStark.sample_indices(t, fiat_shamir, N)];  per index i: the row tuple at x_i, its authentication path, the
    opening of g (the element g[i] and its path; with coset leaves the tuple of leaf i mod (N / a) and its one path);
    then Fri.prove over g.

Opening each polynomial at its own points (include/bfstark_open.h):
      .open_at(commitment, plan, proof_stream)        plan: groups (row columns, points), see OpeningPlan; returns values[g][j][r]
      .verify_at(root, plan, values, proof_stream)    host only
With base[g][j] a running count over the pairs in plan order, raised by |columns_g| per pair:

    g(x) = sum_g sum_j ( lambda^base[g][j] * S_g(x) - Y_{g,j} ) / (x - z_{g,j}),   S_g = sum_r lambda^r f_{columns_g[r]},
    Y_{g,j} = sum_r lambda^(base[g][j] + r) y_{g,j,r}

-- for one group of all columns the formula above word for word.  Proof stream of `open_at`, after the root: the DISTINCT points in order
of first appearance (a list of elements); the plan's shape (a list per group of (tuple(columns), tuple(point indices)), plain ints, so that
the plan is inside every later Fiat-Shamir hash); the values (a list per group of a list per point of a list per column); from lambda on
exactly as `open`.

Opening the polynomials of several commitments with one proof (include/bfstark_rounds.h):
      .open_rounds(commitments, plan, proof_stream)              1..4 Commitments of this PolynomialCommitment; returns values[g][j][r]
      .verify_rounds(roots, widths, plan, values, proof_stream)  host only; widths = the commitments' row widths
      .global_column(commitments, r, c)                          row column c of commitments[r] in the plan's numbering
The commitments are made at any moments of one transcript (each `commit` pushes its root; the caller pushes, pulls and draws challenges in
between).  Their row columns are numbered through, first[r] = m_0 + .. + m_{r-1}, M = sum m_r <= 96, and the plan is an OpeningPlan over
the M columns with wider limits (24 groups, 24 distinct points, 48 pairs, 32 columns in any one group); a group may hold columns of
different commitments.  g is the formula above with M in the place of m.  Proof stream of `open_rounds` (all roots are in the stream
already): the distinct points in order of first appearance; the shape (tuple(widths), [(tuple(columns), tuple(point indices)) per
group]), plain ints -- numbering and plan are inside every later Fiat-Shamir hash; the values; [lambda]; the root of the tree over g;
[t indices]; per index i: for r = 0 .. R - 1 the row tuple of C_r at x_i and its authentication path, then the opening of g as above;
then Fri.prove over g.  With one commitment the quotient is `open_at`'s and the stream differs by the widths in the shape.

For a protocol whose codewords exist already, and whose verifier learns the values from the proof (BrainfuckStark.prove_deep / verify_deep):
      .commit_evaluated(polys, codewords, proof_stream)          `commit` over codewords that are in HBM in Commitment's layout: nothing is transformed
      .read_rounds(roots, widths, plan, proof_stream)            `verify_rounds` that TAKES the values from the stream -> values[g][j][r] or None

The three openings are ONE prover and ONE verifier over an OpeningPlan (PolynomialCommitment._open, ._verify_quotient): `open` is the plan
of one group of all columns (built without the rule against a point given twice, which `open` never had), `open_at` a plan over one
commitment, `open_rounds` a plan over the columns of several.  They differ in what they push behind the points (nothing; the shape; the
widths and the shape), in the shape of the values in the stream (`open` has no group level) and in the library entry that builds g
(bfs_deep_quotient, which is cheaper for one group; bfsx_deep_quotient_groups; bfsr_deep_quotient_rounds) -- ._quotient marshals the plan
for all three.  The verifiers differ in how they compare points, header and values with the caller's.
"""
import collections
import ctypes
import functools
from hashlib import blake2b

import numpy as np

from . import _lib
from .air import P, xadd, xinv, xmul, xsub
from .algebra import BaseFieldElement
from .arrays import BaseArray, XArray, raw_ntt
from .device import DeviceBuffer, current_stream, gather
from .extension_field import ExtensionFieldElement
from .merkle import CosetMerkle, Merkle, leaf_pickle_source
from .ntt import _base_value
from .salted_merkle import SaltedMerkle, ZippedSaltedMerkle

_u64 = ctypes.c_uint64
MAX_POINTS_PER_LAUNCH = 4          # bfs_poly_eval_points, bfs_deep_quotient
MAX_COLUMNS, MAX_EXT_COLUMNS = 32, 16   # bfs_merkle_build_rows
MAX_COLUMNS_PER_EVALUATION = 96    # bfsx_poly_eval_columns
MAX_GROUPS, MAX_PLAN_POINTS, MAX_PAIRS = 8, 8, 16   # bfsx_deep_quotient_groups: an opening plan
MAX_COMMITMENTS = 4                # open_rounds
PlanLimits = collections.namedtuple("PlanLimits", "groups points pairs columns group_columns")
PLAN_LIMITS = PlanLimits(MAX_GROUPS, MAX_PLAN_POINTS, MAX_PAIRS, MAX_COLUMNS, MAX_COLUMNS)      # one commitment: one launch
ROUNDS_LIMITS = PlanLimits(24, 24, 48, 96, MAX_COLUMNS)                                         # bfsr_deep_quotient_rounds


def _limbs(z):
    """(c0, c1, c2) of an ExtensionFieldElement, a BaseFieldElement, an int or a limb triple"""
    if isinstance(z, ExtensionFieldElement):
        return tuple(z.limbs())
    if isinstance(z, BaseFieldElement):
        return (z.value % P, 0, 0)
    if isinstance(z, (tuple, list)):
        return tuple(int(v) % P for v in z)
    return (int(z) % P, 0, 0)


def _times_x(a):
    """a * X in F_p[X]/(X^3 - X + 1)"""
    return (-a[2] % P, (a[0] + a[2]) % P, a[1])


def _point_chunks(points):
    return [points[first:first + MAX_POINTS_PER_LAUNCH] for first in range(0, len(points), MAX_POINTS_PER_LAUNCH)]


def _flat_points(points):
    return (_u64 * (3 * len(points)))(*[v for z in points for v in z])


def _eval_requests(requests):
    """requests: (columns, points), columns a list of (ptr, n) SEPARATE base-coefficient arrays -> per request values[b][j] = limb
    triple of column b at point j: bfsx_poly_eval_columns, one call per 96 columns and four points, every call enqueued before the ONE
    read-back of all results"""
    lib, stream = _lib.load(), current_stream()
    out = DeviceBuffer(3 * sum(len(columns) * len(points) for columns, points in requests))
    at, calls = 0, []
    for r, (columns, points) in enumerate(requests):
        for first in range(0, len(columns), MAX_COLUMNS_PER_EVALUATION):
            some = columns[first:first + MAX_COLUMNS_PER_EVALUATION]
            table = (_lib.EvalColumn * len(some))(*[_lib.EvalColumn(ptr, n) for ptr, n in some])
            for j0, chunk in enumerate(_point_chunks(points)):
                _lib.check(lib.bfsx_poly_eval_columns(table, len(some), _flat_points(chunk), len(chunk), out.ptr + 8 * at, stream))
                calls.append((r, first, len(some), j0 * MAX_POINTS_PER_LAUNCH, len(chunk), at))
                at += 3 * len(some) * len(chunk)
    words = [int(v) for v in out.to_numpy()]
    out.free()
    results = [[[None] * len(points) for _ in columns] for columns, points in requests]
    for r, first, count, j0, k, at in calls:
        for b in range(count):
            for j in range(k):
                w = at + 3 * (b * k + j)
                results[r][first + b][j0 + j] = tuple(words[w:w + 3])
    return results


def _eval_columns(ptr, n, stride, batch, points):
    """one strided buffer of `batch` columns of equal length -> [[limb triple of column b at point j] per column] per point:
    bfs_poly_eval_points, four points per launch, every launch enqueued before the ONE read-back"""
    lib, stream = _lib.load(), current_stream()
    out = DeviceBuffer(3 * len(points) * batch)
    at = 0
    for chunk in _point_chunks(points):
        _lib.check(lib.bfs_poly_eval_points(ptr, n, stride, batch, _flat_points(chunk), len(chunk), out.ptr + 8 * at, stream))
        at += 3 * batch * len(chunk)
    words = [int(v) for v in out.to_numpy()]
    out.free()
    values, at = [[None] * batch for _ in points], 0
    for first, chunk in enumerate(_point_chunks(points)):
        for b in range(batch):
            for j in range(len(chunk)):
                values[first * MAX_POINTS_PER_LAUNCH + j][b] = tuple(words[at:at + 3])
                at += 3
    return values


def _combine_planes(v):
    """v0 + X v1 + X^2 v2 for the values of an extension polynomial's three limb columns"""
    return xadd(v[0], xadd(_times_x(v[1]), _times_x(_times_x(v[2]))))


def evaluate_at(coeffs, points, xfield=None):
    """f(z) for every z of `points` (ExtensionFieldElements; BaseFieldElements and ints are lifted), f given by coefficients in HBM.
    coeffs: an XArray, or a BaseArray -- of batch 1: a list with one ExtensionFieldElement per point; of batch b > 1: per point a list
    of the b columns' values.  The coefficients are read once per four points and nothing but the 3 k (b) result words leaves HBM."""
    from .extension_field import ExtensionField
    pts = [_limbs(z) for z in points]
    xf = xfield or next((z.field for z in points if isinstance(z, ExtensionFieldElement)), None) or (coeffs.field if isinstance(coeffs, XArray) else ExtensionField.main())
    if not pts:
        return []
    assert len(coeffs) >= 1, "evaluate_at: no coefficients (the zero polynomial is one zero coefficient)"
    if isinstance(coeffs, XArray):
        raw = _eval_columns(coeffs.ptr, coeffs.n, coeffs.stride, 3, pts)
        return [xf.from_limbs(_combine_planes(v)) for v in raw]
    assert isinstance(coeffs, BaseArray), "evaluate_at takes a BaseArray or an XArray"
    raw = _eval_columns(coeffs.ptr, coeffs.n, coeffs.n, coeffs.batch, pts)
    if coeffs.batch == 1:
        return [xf.from_limbs(v[0]) for v in raw]
    return [[xf.from_limbs(c) for c in v] for v in raw]


class _RowCount:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


class Commitment:
    """what `commit` returns: coefficients, codewords and the row tree, all in HBM"""

    def __init__(self, polys, is_ext, order, codewords, n, tree):
        self.polys, self.is_ext, self.order, self.codewords, self.n, self.tree = polys, is_ext, order, codewords, n, tree
        self.n_ext = sum(is_ext)
        self.n_base = len(polys) - self.n_ext
        self._rows = {}

    def root(self):
        return self.tree.root()

    def column_of(self, position):
        """the row column of the polynomial at `position` of the list `commit` was given (the inverse of `order`)"""
        return self.order.index(position)

    def column_ptr(self, c):
        """first word of column c of the row (extension columns first)"""
        return self.codewords.ptr + 8 * self.n * (3 * c if c < self.n_ext else 3 * self.n_ext + (c - self.n_ext))

    def row_requests(self, i):
        reqs = [(self.column_ptr(c) + 8 * i, 3, self.n) for c in range(self.n_ext)]
        if self.n_base:
            reqs.append((self.column_ptr(self.n_ext) + 8 * i, self.n_base, self.n))
        return reqs


class OpeningPlan:
    """a checked opening plan: which row columns are opened where.  plan: a list of groups (columns_g, points_g) -- columns_g an
    ascending, non-empty list of row columns, every column 0 .. m - 1 in exactly one group; points_g 1..4 pairwise different points
    outside the domain (equal limb triples are one point; the same point may serve several groups).  At most 8 groups, 8 distinct
    points, 16 (group, point) pairs, 32 columns -- or what `limits` (a PlanLimits) says: ROUNDS_LIMITS for a plan over the columns of
    several commitments (24 groups, 24 distinct points, 48 pairs, 96 columns, 32 in any one group).  Anything else raises ValueError
    with the reason -- before any GPU work.  distinct=False (the one group of `open`) takes the points as they come: a point given twice is
    two points of the plan.

        points      the distinct points as limb triples, in order of first appearance
        groups      per group (columns, indices into `points`)
        base        base[g][j]: the exponent of lambda at which pair (g, j) starts (a running count of the pairs' columns)
        shape       what the proof stream carries: per group (tuple(columns), tuple(point indices)), plain ints"""

    def __init__(self, plan, in_domain, m=None, limits=PLAN_LIMITS, distinct=True):
        try:
            groups = [([int(c) for c in columns], [_limbs(z) for z in points]) for columns, points in plan]
        except (TypeError, ValueError):
            raise ValueError("an opening plan is a list of (columns, points) groups")
        if not 1 <= len(groups) <= limits.groups:
            raise ValueError("an opening plan has 1 .. %d groups (got %d)" % (limits.groups, len(groups)))
        self.points, self.groups, self.base = [], [], []
        seen, count = set(), 0
        for g, (columns, points) in enumerate(groups):
            own = set(columns)
            if not columns or columns != sorted(own) or columns[0] < 0:
                raise ValueError("group %d: columns must be an ascending, non-empty list of row columns" % g)
            if seen & own:
                raise ValueError("group %d: column %d lies in an earlier group too" % (g, min(seen & own)))
            seen |= own
            if len(columns) > limits.group_columns:
                raise ValueError("group %d: at most %d columns in a group (got %d)" % (g, limits.group_columns, len(columns)))
            if not 1 <= len(points) <= MAX_POINTS_PER_LAUNCH or any(len(z) != 3 for z in points):
                raise ValueError("group %d: 1 .. %d points of three limbs each" % (g, MAX_POINTS_PER_LAUNCH))
            if distinct and len(set(points)) != len(points):
                raise ValueError("group %d: a point appears twice" % g)
            indices = []
            for z in points:
                if in_domain(z):
                    raise ValueError("cannot open at a point of the FRI domain: %s" % (z,))
                if not distinct or z not in self.points:
                    self.points.append(z)
                indices.append(len(self.points) - 1 if not distinct else self.points.index(z))
            self.groups.append((columns, indices))
            self.base.append([count + j * len(columns) for j in range(len(points))])
            count += len(points) * len(columns)
        self.m, self.exponents = len(seen), count
        self.pairs = sum(len(indices) for _, indices in self.groups)
        if seen != set(range(self.m)) or (m is not None and self.m != m):
            raise ValueError("the groups must hold every column 0 .. %d exactly once" % ((self.m if m is None else m) - 1))
        if self.m > limits.columns:
            raise ValueError("at most %d columns (got %d)" % (limits.columns, self.m))
        if len(self.points) > limits.points:
            raise ValueError("at most %d distinct points (got %d)" % (limits.points, len(self.points)))
        if self.pairs > limits.pairs:
            raise ValueError("at most %d (group, point) pairs (got %d)" % (limits.pairs, self.pairs))
        self.shape = [(tuple(columns), tuple(indices)) for columns, indices in self.groups]

    def combined_values(self, values, lam):
        """Y[g][j] = sum_r lambda^(base[g][j] + r) y_{g,j,r}; also the powers of lambda it used"""
        powers = [(1, 0, 0)]
        for _ in range(self.exponents):
            powers.append(xmul(powers[-1], lam))
        combined = []
        for g, per_group in enumerate(values):
            combined.append([])
            for j, per_point in enumerate(per_group):
                acc = (0, 0, 0)
                for r, y in enumerate(per_point):
                    acc = xadd(acc, xmul(powers[self.base[g][j] + r], y))
                combined[-1].append(acc)
        return combined, powers


def _reads_leaf_pickles(verifier):
    """a verifier whose last argument is the proof stream: while it runs, Merkle.verify takes the pickle of an opened leaf from the stream
    that holds it (merkle.leaf_pickle_source) -- unless an outer verifier has said so already"""
    @functools.wraps(verifier)
    def entry(self, *args, **kwargs):
        proof_stream = kwargs["proof_stream"] if "proof_stream" in kwargs else args[-1]
        if leaf_pickle_source.get() is not None or not hasattr(proof_stream, "pickle_of"):
            return verifier(self, *args, **kwargs)
        token = leaf_pickle_source.set(proof_stream.pickle_of)
        try:
            return verifier(self, *args, **kwargs)
        finally:
            leaf_pickle_source.reset(token)
    return entry


class PolynomialCommitment:
    """commit / open / verify over a `Fri` of any mode (folding factor, coset leaves, grinding).

    With N = fri.domain.length, d = N // fri.expansion_factor and t = fri.num_colinearity_tests: polynomials have at most d coefficients
    (a polynomial with more is not what the low-degree test vouches for).  An accepted opening says: the columns behind `root` are
    within the FRI proximity bound of polynomials of degree < d that take the claimed values.

    hiding=True: `commit` / `commit_evaluated` build the SALTED row tree of prove() (ZippedSaltedMerkle: leaf i = blake2b(pickle(row
    tuple) || pickle(salt_i)), 24-byte salts that stay in HBM), every opening pushes `(salt, path)` behind each opened row as
    SaltedMerkle.open returns it, and the verifier checks it with SaltedMerkle.verify (a salt that is not 24 bytes: "opened row is not
    well formed").  The commitment then hides the unopened rows; what the opened rows, the values and g reveal is for the caller to
    blind -- BrainfuckStark.prove_deep(zero_knowledge=True) does ("Zero-knowledge openings": blinded columns and a uniform
    masking polynomial among the committed ones).  hiding=False (the default) keeps every stream as it was.

    What this scheme is NOT:
      * by default it is not hiding -- the row tree is unsalted --, and with or without `hiding` it is not zero-knowledge by itself: no
        randomizer polynomial is mixed into g unless the caller commits to one, the opened rows are plain values of the committed
        polynomials, and the values themselves are in the proof;
      * it does not choose the points -- the caller must draw them AFTER the commitment's root is in the transcript (from
        proof_stream.prover_fiat_shamir()); for points fixed beforehand a prover can commit to polynomials made to fit.
    Points of the FRI domain cannot be opened (the quotient's denominator vanishes there): `open` refuses them."""

    def __init__(self, fri, hiding=False):
        self.fri = fri
        self.hiding = bool(hiding)
        self.xfield = fri.field
        self.n = fri.domain.length
        self.max_coefficients = self.n // fri.expansion_factor
        self.offset, self.omega = _base_value(fri.domain.offset), _base_value(fri.domain.omega)

    # ---------------------------------------------------------------------------------------------------------- shared
    def _base_field(self):
        return self.xfield.modulus.coefficients[0].field          # the BaseField instance the rows' base elements point at

    def in_domain(self, z):
        """is z one of the points offset * omega^i: a lifted base value v with (v / offset)^N = 1"""
        c0, c1, c2 = _limbs(z)
        return c1 == 0 and c2 == 0 and pow(c0 * pow(self.offset, P - 2, P) % P, self.n, P) == 1

    @staticmethod
    def _indices(t, seed, n):
        return [int.from_bytes(blake2b(seed + bytes(i)).digest(), "big") % n for i in range(t)]      # BrainfuckStark.sample_indices

    # ---------------------------------------------------------------------------------------------------------- prover
    def commit(self, polys, proof_stream):
        """polys: BaseArrays (batch 1) and XArrays of coefficients in HBM, at most N // expansion_factor each; at most 32 columns, at
        most 16 of them extension columns.  Extends every polynomial to the FRI domain (bfs_gl_ntt), hashes the rows
        (bfs_merkle_build_rows without salts: leaf i = the tuple of all values at x_i, extension columns first) and pushes the root."""
        stream, n = current_stream(), self.n
        assert polys, "nothing to commit to"
        for f in polys:
            assert isinstance(f, XArray) or (isinstance(f, BaseArray) and f.batch == 1), "polynomials are BaseArrays of batch 1 and XArrays"
            assert 1 <= len(f) <= self.max_coefficients, "a polynomial has 1 .. N / expansion_factor coefficients"
        is_ext = [isinstance(f, XArray) for f in polys]
        order = [i for i, e in enumerate(is_ext) if e] + [i for i, e in enumerate(is_ext) if not e]
        n_ext = sum(is_ext)
        assert len(polys) <= MAX_COLUMNS and n_ext <= MAX_EXT_COLUMNS, "at most 32 columns, at most 16 extension columns"
        codewords = DeviceBuffer((3 * n_ext + len(polys) - n_ext) * n)
        committed = Commitment(list(polys), is_ext, order, codewords, n, None)
        log_n = n.bit_length() - 1
        cols = (_lib.RowColumn * len(polys))()
        for c, position in enumerate(order):
            f = polys[position]
            if is_ext[position]:
                raw_ntt(f.ptr, f.n, f.stride, committed.column_ptr(c), n, log_n, 3, self.omega, self.offset, 1, stream)
            else:
                raw_ntt(f.ptr, f.n, f.n, committed.column_ptr(c), n, log_n, 1, self.omega, self.offset, 1, stream)
            cols[c].d_values, cols[c].is_ext, cols[c].field_id = committed.column_ptr(c), int(is_ext[position]), 1
        return self._commit_rows(committed, cols, proof_stream)

    def _commit_rows(self, committed, cols, proof_stream):
        """the row tree over a commitment's codewords (bfs_merkle_build_rows without salts); pushes the root.  hiding: the salted row
        tree of prove() instead (ZippedSaltedMerkle: 24 bytes of salt per leaf, made on the device from one 32-byte draw and kept there,
        or taken from a replaced random source)"""
        if self.hiding:
            committed.tree = ZippedSaltedMerkle([(c.d_values, c.is_ext, c.field_id) for c in cols], self.n, lambda i: None)
            proof_stream.push(committed.tree.root())
            return committed
        nodes = DeviceBuffer(2 * self.n * 8)
        _lib.check(_lib.load().bfs_merkle_build_rows(cols, len(committed.polys), self.n, None, 0, nodes.ptr, current_stream()))
        committed.tree = Merkle(_RowCount(self.n), _device_nodes=nodes)
        proof_stream.push(committed.tree.root())
        return committed

    def commit_evaluated(self, polys, codewords, proof_stream):
        """`commit` for polynomials whose codewords on the FRI domain are in HBM already: nothing is transformed.  codewords: a device
        buffer in Commitment's layout -- per extension polynomial three planes of N words, then per base polynomial N words --, which
        the commitment keeps and never writes; polys: the coefficients in THAT order (XArrays, with any stride, then BaseArrays of batch 1),
        which openings evaluate.  That the codewords are the polynomials' is the caller's word: an opening of other data fails its own
        low-degree test.  Builds the row tree and pushes the root, as `commit` does."""
        n = self.n
        assert polys, "nothing to commit to"
        is_ext = [isinstance(f, XArray) for f in polys]
        for f in polys:
            assert isinstance(f, XArray) or (isinstance(f, BaseArray) and f.batch == 1), "polynomials are BaseArrays of batch 1 and XArrays"
            assert 1 <= len(f) <= self.max_coefficients, "a polynomial has 1 .. N / expansion_factor coefficients"
        assert is_ext == sorted(is_ext, reverse=True), "extension polynomials first: the order of the codewords in the buffer"
        n_ext = sum(is_ext)
        assert len(polys) <= MAX_COLUMNS and n_ext <= MAX_EXT_COLUMNS, "at most 32 columns, at most 16 extension columns"
        assert codewords.count >= (3 * n_ext + len(polys) - n_ext) * n, "the codeword buffer is shorter than the row layout"
        committed = Commitment(list(polys), is_ext, list(range(len(polys))), codewords, n, None)
        cols = (_lib.RowColumn * len(polys))()
        for c in range(len(polys)):
            cols[c].d_values, cols[c].is_ext, cols[c].field_id = committed.column_ptr(c), int(is_ext[c]), 1
        return self._commit_rows(committed, cols, proof_stream)

    def _row(self, committed, i, words):
        """the tuple of element objects of row i (one object per row: a row opened twice is the same tuple twice)"""
        if i not in committed._rows:
            xf, base = self.xfield, self._base_field()
            ext = [xf.from_limbs([int(v) for v in words[3 * c:3 * c + 3]]) for c in range(committed.n_ext)]
            committed._rows[i] = tuple(ext + [BaseFieldElement(int(v), base) for v in words[3 * committed.n_ext:]])
        return committed._rows[i]

    # every opening is an OpeningPlan over the row columns of a list of commitments, numbered through: `open` one group of all columns of
    # one commitment, `open_at` a plan over one commitment, `open_rounds` a plan over several
    def _one_group(self, points, m):
        """the plan of `open`, `verify` and `quotient`: all m columns at `points` as they come (a point given twice stays two points;
        whether a point lies in the domain is for the caller to ask, as it was: `open` and `verify` do, `quotient` never did)"""
        return OpeningPlan([(range(m), points)], lambda z: False, m, PlanLimits(1, MAX_POINTS_PER_LAUNCH, MAX_POINTS_PER_LAUNCH, m, m), distinct=False)

    @staticmethod
    def _where(commitments):
        """per column of the through numbering: (its commitment, its row column there)"""
        return [(committed, c) for committed in commitments for c in range(len(committed.polys))]

    def _quotient(self, entry, arguments, commitments, plan, values, lam, tail=()):
        """the DEEP quotient codeword (XArray) of a plan by one of the three entries.  values[g][j][r]: limb triples; arguments(plan, Y):
        how the entry takes the plan between omega and lambda; tail: what it takes between the output and the stream"""
        n, where = self.n, self._where(commitments)
        cols = (_lib.RowColumn * len(where))()
        for at, column in enumerate(c for columns, _ in plan.groups for c in columns):      # (the kernels want the columns in group order)
            committed, c = where[column]
            cols[at].d_values, cols[at].is_ext, cols[at].field_id = committed.column_ptr(c), int(c < committed.n_ext), 1
        combined, _ = plan.combined_values(values, lam)
        g = XArray.empty(n, self.xfield)
        _lib.check(entry(cols, len(where), n, n.bit_length() - 1, self.offset, self.omega, *arguments(plan, combined), (_u64 * 3)(*lam), g.ptr, g.stride,
                         *tail, current_stream()))
        return g

    @staticmethod
    def _group_arguments(plan, combined):
        """bfs_deep_quotient: the points of the one group and its Y_j"""
        return _flat_points(plan.points), _flat_points(combined[0]), len(plan.points)

    @staticmethod
    def _plan_arguments(plan, combined):
        """both plan entries: group sizes, the distinct points, per pair its point and its Y"""
        u32, groups = ctypes.c_uint32, len(plan.groups)
        return ((u32 * groups)(*[len(columns) for columns, _ in plan.groups]), (u32 * groups)(*[len(indices) for _, indices in plan.groups]), groups,
                _flat_points(plan.points), len(plan.points), (u32 * plan.pairs)(*[p for _, indices in plan.groups for p in indices]),
                _flat_points([y for per_group in combined for y in per_group]))

    def quotient(self, committed, points, values, lam):
        """the DEEP quotient codeword (XArray) of the commitment's columns: bfs_deep_quotient (its own kernel: one group costs less there,
        profiles/pcs.md).  points: limb triples; values[j][p]: limb triples"""
        return self._quotient(_lib.load().bfs_deep_quotient, self._group_arguments, [committed], self._one_group(points, len(committed.polys)), [values], lam)

    def _open(self, commitments, plan, header, quotient, proof_stream, pushed=lambda values: values):
        """THE prover: the plan's points, `header` (what this opening pushes behind them), the values (evaluated here; pushed(values) is
        what the stream gets), lambda, g = quotient(commitments, plan, values as limb triples, lambda), and what follows lambda in every
        opening.  -> values[g][j][r]"""
        xf = self.xfield
        proof_stream.push([xf.from_limbs(z) for z in plan.points])
        for part in header:
            proof_stream.push(part)
        raw, values = self._plan_values(plan, commitments)
        proof_stream.push(pushed(values))
        lam = tuple(xf.sample(proof_stream.prover_fiat_shamir()).limbs())
        self._prove_quotient(commitments, quotient(commitments, plan, raw, lam), proof_stream)
        return values

    def open(self, committed, points, proof_stream):
        """proves the values of every committed polynomial at `points` (1..4 ExtensionFieldElements outside the FRI domain); returns
        them: a list per point of a list per polynomial IN ROW ORDER -- extension polynomials first, then base polynomials, each group in
        the order `commit` was given them (Commitment.order[c] = position of row column c in that list)"""
        assert 1 <= len(points) <= MAX_POINTS_PER_LAUNCH, "1 .. 4 points per opening"
        for z in points:
            if self.in_domain(z):
                raise ValueError("cannot open at a point of the FRI domain: %s" % (z,))
        one = functools.partial(self._quotient, _lib.load().bfs_deep_quotient, self._group_arguments)
        return self._open([committed], self._one_group(points, len(committed.polys)), [], one, proof_stream, lambda values: values[0])[0]

    def _prove_quotient(self, commitments, g, proof_stream):
        """what follows lambda in every opening: the root of the tree over g, the t consistency indices with their rows (one row and
        one path per commitment of the list, in its order) and openings of g, then Fri.prove over g"""
        xf, n, t, fri = self.xfield, self.n, self.fri.num_colinearity_tests, self.fri
        coset = fri.coset_leaves
        a = fri.folding_factor if coset else 1
        q = n // a
        g_tree = CosetMerkle(g, a) if coset else Merkle(g)
        proof_stream.push(g_tree.root())
        indices = self._indices(t, proof_stream.prover_fiat_shamir(), n)
        # everything the openings read from HBM in one round trip
        rows = list(dict.fromkeys(indices))
        leaves = list(dict.fromkeys(i % q for i in indices))
        requests, spans = [], {}
        for i in rows:
            for r, committed in enumerate(commitments):
                reqs = committed.row_requests(i)
                spans["row", r, i] = (len(requests), len(reqs))
                requests += reqs
        salted = []
        if self.hiding:          # salts made on the device come with the same round trip; tree.open then knows them
            for committed in commitments:
                reqs, store = committed.tree.salt_requests(rows)
                salted.append((store, len(requests), len(reqs)))
                requests += reqs
        for c in leaves:
            spans["leaf", c] = (len(requests), a)
            requests += [(g.ptr + 8 * (c + j * q), 3, g.stride) for j in range(a)]
        fetched = gather(requests)
        starts = np.concatenate([[0], np.cumsum([r[1] for r in requests])])

        def words(key):
            first, count = spans[key]
            return fetched[starts[first]:starts[first + count]]
        for store, first, count in salted:
            store([fetched[starts[first + j]:starts[first + j + 1]] for j in range(count)])
        known = {}
        for i in indices:
            for r, committed in enumerate(commitments):
                proof_stream.push(self._row(committed, i, words(("row", r, i))))
                proof_stream.push(committed.tree.open(i))
            c = i % q
            if c not in known:
                w = [int(v) for v in words(("leaf", c))]
                elements = [xf.from_limbs(w[3 * j:3 * j + 3]) for j in range(a)]
                known[c] = tuple(elements) if coset else elements[0]
            proof_stream.push(known[c])
            proof_stream.push(g_tree.open(c))
        if coset:
            fri.prove(g, proof_stream, round0_tree=g_tree)
        else:
            fri.prove(g, proof_stream, known_leafs=known or None, round0_tree=g_tree)

    # ---------------------------------------------------------------------------------------------------------- verifier (host only)
    @_reads_leaf_pickles
    def verify(self, root, points, values, proof_stream):
        """does the proof in `proof_stream` (read position right behind the commitment's root) show that the polynomials behind `root`
        take `values` (what `open` returned: a list per point of a list per polynomial in row order) at `points`?
        Host code only: Python ints, hashlib and Fri.verify; one printed line per refusal."""
        is_element = lambda e: isinstance(e, ExtensionFieldElement)
        pts = [_limbs(z) for z in points]
        if not 1 <= len(pts) <= MAX_POINTS_PER_LAUNCH or any(self.in_domain(z) for z in pts):
            print("points cannot be opened")
            return False
        pushed = proof_stream.pull()
        if not isinstance(pushed, list) or not all(is_element(z) for z in pushed) or [_limbs(z) for z in pushed] != pts:
            print("points differ from the caller's")
            return False
        claimed = proof_stream.pull()
        want = [[_limbs(v) for v in per_point] for per_point in values]
        m = len(want[0]) if want else 0
        if (not isinstance(claimed, list) or len(claimed) != len(want) or m < 1 or any(len(w) != m for w in want)
                or not all(isinstance(c, list) and len(c) == m and all(is_element(v) for v in c) for c in claimed)
                or [[_limbs(v) for v in c] for c in claimed] != want):
            print("values differ from the caller's")
            return False
        return self._verify_quotient([(root, m)], self._one_group(pts, m), [want], proof_stream)

    def _verify_quotient(self, trees, plan, want, proof_stream):
        """THE verifier, once points, header and values are the caller's: lambda, then what follows it (_check_quotient) against the
        plan's formula.  want[g][j][r]: limb triples"""
        lam = tuple(self.xfield.sample(proof_stream.verifier_fiat_shamir()).limbs())
        combined, powers = plan.combined_values(want, lam)
        return self._check_quotient(trees, lambda i, row: self._plan_quotient_at(i, row, plan, combined, powers), proof_stream)

    def _check_quotient(self, trees, quotient_at, proof_stream):
        """what follows lambda in every opening, read back.  trees: (root, width) per commitment, in the order their rows were pushed;
        quotient_at(i, the rows at x_i one behind the other, as limb triples) is g[i] as the statement has it"""
        n, t, fri = self.n, self.fri.num_colinearity_tests, self.fri
        is_element = lambda e: isinstance(e, ExtensionFieldElement)
        g_root = proof_stream.pull()
        if not isinstance(g_root, (bytes, bytearray)):
            print("quotient root is not a digest")
            return False
        indices = self._indices(t, proof_stream.verifier_fiat_shamir(), n)
        coset = fri.coset_leaves
        a = fri.folding_factor if coset else 1
        q = n // a
        # a row has its extension columns first; how many there are is read off the first row and must hold for every row
        shapes = [None] * len(trees)
        for i in indices:
            rows = []
            for r, (root, m) in enumerate(trees):
                row = proof_stream.pull()
                if not isinstance(row, tuple) or len(row) != m or not all(is_element(e) or isinstance(e, BaseFieldElement) for e in row):
                    print("opened row is not well formed")
                    return False
                kinds = [is_element(e) for e in row]
                if kinds != sorted(kinds, reverse=True) or (shapes[r] is not None and kinds != shapes[r]):
                    print("opened row is not well formed")
                    return False
                shapes[r] = kinds
                path = proof_stream.pull()
                if self.hiding:          # (salt, path) as SaltedMerkle.open returns it
                    if (not isinstance(path, tuple) or len(path) != 2 or not isinstance(path[0], (bytes, bytearray)) or len(path[0]) != 24
                            or not self._is_path(path[1], n)):
                        print("opened row is not well formed")
                        return False
                    authentic = SaltedMerkle.verify(root, i, path[0], path[1], row)
                else:
                    authentic = self._is_path(path, n) and Merkle.verify(root, i, path, row)
                if not authentic:
                    print("merkle authentication path verification fails for an opened row")
                    return False
                rows += [_limbs(e) for e in row]
            leaf = proof_stream.pull()
            path = proof_stream.pull()
            c = i % q
            if coset:
                well_formed = isinstance(leaf, tuple) and len(leaf) == a and all(is_element(e) for e in leaf)
            else:
                well_formed = is_element(leaf)
            if not well_formed or not self._is_path(path, q) or not Merkle.verify(g_root, c, path, leaf):
                print("merkle authentication path verification fails for the quotient")
                return False
            opened = _limbs(leaf[i // q] if coset else leaf)
            if opened != quotient_at(i, rows):
                print("quotient does not match the opened row")
                return False
        if not fri.verify(proof_stream, g_root):
            print("low-degree test of the quotient fails")
            return False
        return True

    @staticmethod
    def _is_path(path, leaves):
        return (isinstance(path, list) and len(path) == leaves.bit_length() - 1
                and all(isinstance(node, (bytes, bytearray)) for node in path))

    # ---------------------------------------------------------------------------------------------------------- opening plans
    def plan(self, plan, m=None):
        """the checked OpeningPlan of a list of (columns, points) groups (ValueError with the reason otherwise)"""
        return plan if isinstance(plan, OpeningPlan) else OpeningPlan(plan, self.in_domain, m)

    def quotient_at(self, committed, plan, values, lam):
        """the DEEP quotient codeword (XArray) of an opening plan: bfsx_deep_quotient_groups.  values[g][j][r]: limb triples"""
        return self._quotient(_lib.load().bfsx_deep_quotient_groups, self._plan_arguments, [committed], plan, values, lam)

    def open_at(self, committed, plan, proof_stream):
        """proves, for every group (columns_g, points_g) of `plan` (see OpeningPlan), the values of the row columns columns_g at the
        points points_g; returns them as values[g][j][r] = f_{columns_g[r]}(points_g[j]).  Commitment.column_of(position) is the row
        column of the polynomial at `position` of the list `commit` was given.  The plan is checked before any GPU work (ValueError)."""
        plan = self.plan(plan, len(committed.polys))
        return self._open([committed], plan, [plan.shape], functools.partial(self._quotient, _lib.load().bfsx_deep_quotient_groups, self._plan_arguments),
                          proof_stream)

    def _plan_values(self, plan, commitments):
        """the values a plan over the columns of `commitments` asks for, as limb triples and as elements, both [g][j][r].  One evaluation
        call per distinct point set: the coefficient columns of every group that is opened there"""
        xf, where = self.xfield, self._where(commitments)
        point_sets = list(dict.fromkeys(tuple(indices) for _, indices in plan.groups))
        requests, places = [], {}
        for point_set in point_sets:
            coefficient_columns = []
            for g, (columns, indices) in enumerate(plan.groups):
                if tuple(indices) == point_set:
                    for r, c in enumerate(columns):
                        committed, row_column = where[c]
                        f = committed.polys[committed.order[row_column]]
                        planes = [(f.ptr + 8 * l * f.stride, f.n) for l in range(3)] if isinstance(f, XArray) else [(f.ptr, f.n)]
                        places[g, r] = (len(requests), len(coefficient_columns), len(planes))
                        coefficient_columns += planes
            requests.append((coefficient_columns, [plan.points[p] for p in point_set]))
        got = _eval_requests(requests)
        raw = []
        for g, (columns, indices) in enumerate(plan.groups):
            raw.append([[None] * len(columns) for _ in indices])
            for r in range(len(columns)):
                request, first, planes = places[g, r]
                for j in range(len(indices)):
                    v = [got[request][first + l][j] for l in range(planes)]
                    raw[g][j][r] = _combine_planes(v) if planes == 3 else v[0]
        return raw, [[[xf.from_limbs(v) for v in per_point] for per_point in per_group] for per_group in raw]

    @_reads_leaf_pickles
    def verify_at(self, root, plan, values, proof_stream):
        """does the proof in `proof_stream` (read position right behind the commitment's root) show that the polynomials behind `root`
        take `values` (what `open_at` returned: values[g][j][r]) under `plan`?  Host code only: Python ints, hashlib and Fri.verify; one
        printed line per refusal."""
        try:
            plan = self.plan(plan)
        except ValueError as e:
            print("plan cannot be opened: %s" % e)
            return False
        return self._verify_plan([(root, plan.m)], plan, plan.shape, values, proof_stream)

    def _verify_plan(self, trees, plan, shape, values, proof_stream, read=False):
        """what verify_at, verify_rounds and read_rounds share: points, shape and values against the caller's, then the quotient.  trees:
        (root, width) per commitment; shape: what the prover pushed behind the points.  read (read_rounds): `values` is not looked at;
        the stream's values are checked against the quotient and returned as limb triples values[g][j][r], None on refusal"""
        is_element = lambda e: isinstance(e, ExtensionFieldElement)
        refused = None if read else False
        pushed = proof_stream.pull()
        if not isinstance(pushed, list) or not all(is_element(z) for z in pushed) or [_limbs(z) for z in pushed] != plan.points:
            print("points differ from the caller's plan")
            return refused
        if proof_stream.pull() != shape:
            print("groups differ from the caller's plan")
            return refused
        claimed = proof_stream.pull()
        lengths = [[len(columns)] * len(indices) for columns, indices in plan.groups]
        got = None          # the stream's values as limb triples, if they are lists of lists of lists of elements
        if isinstance(claimed, list) and all(isinstance(per_group, list) and all(isinstance(per_point, list) and all(is_element(v) for v in per_point)
                                                                                 for per_point in per_group) for per_group in claimed):
            got = [[[_limbs(v) for v in per_point] for per_point in per_group] for per_group in claimed]
        if read:
            # the caller does not know the values: they are the stream's, provided they have the plan's shape and are canonical elements
            if got is None or [[len(per_point) for per_point in per_group] for per_group in got] != lengths:
                print("values do not have the shape of the caller's plan")
                return None
            if not all(len(v) == 3 and all(type(c) is int and 0 <= c < P for c in v) for per_group in got for per_point in per_group for v in per_point):
                print("values are not canonical elements")
                return None
            return got if self._verify_quotient(trees, plan, got, proof_stream) else None
        try:
            want = [[[_limbs(v) for v in per_point] for per_point in per_group] for per_group in values]
        except TypeError:
            want = None
        if want is None or [[len(per_point) for per_point in per_group] for per_group in want] != lengths or got != want:
            print("values differ from the caller's")
            return False
        return self._verify_quotient(trees, plan, want, proof_stream)

    def _plan_quotient_at(self, i, row, plan, combined, powers):
        """g[i] from the row at x_i: sum_g sum_j (lambda^base[g][j] S_g - Y_{g,j}) / (x_i - z_{g,j})"""
        x = self.offset * pow(self.omega, i, P) % P
        inverse = [xinv(xsub((x, 0, 0), z)) for z in plan.points]
        g = (0, 0, 0)
        for (columns, indices), base, ys in zip(plan.groups, plan.base, combined):
            s = (0, 0, 0)
            for r, c in enumerate(columns):
                s = xadd(s, xmul(powers[r], row[c]))
            for p, b, y in zip(indices, base, ys):
                g = xadd(g, xmul(xsub(xmul(powers[b], s), y), inverse[p]))
        return g

    # ---------------------------------------------------------------------------------------------------------- openings across commitments
    @staticmethod
    def _widths(widths):
        """the checked list of row widths of 1 .. 4 commitments (ValueError with the reason otherwise)"""
        try:
            widths = [int(w) for w in widths]
        except (TypeError, ValueError):
            raise ValueError("widths: one row width per commitment")
        if not 1 <= len(widths) <= MAX_COMMITMENTS:
            raise ValueError("1 .. %d commitments (got %d)" % (MAX_COMMITMENTS, len(widths)))
        if not all(1 <= w <= MAX_COLUMNS for w in widths):
            raise ValueError("a commitment has 1 .. %d columns (got %s)" % (MAX_COLUMNS, widths))
        return widths

    @staticmethod
    def global_column(commitments, r, c):
        """the column of an `open_rounds` plan that is row column c of commitments[r]: the columns of all commitments are numbered
        through in the order of the list.  commitments: Commitments, or their row widths"""
        widths = [w if isinstance(w, int) else len(w.polys) for w in commitments]
        if not 0 <= r < len(widths) or not 0 <= c < widths[r]:
            raise ValueError("commitment %d has no row column %d" % (r, c))
        return sum(widths[:r]) + c

    def rounds_plan(self, plan, widths):
        """the checked OpeningPlan over the columns of commitments of these row widths (the wider limits: ROUNDS_LIMITS)"""
        m = sum(widths)
        if isinstance(plan, OpeningPlan):
            if plan.m != m:
                raise ValueError("the groups must hold every column 0 .. %d exactly once" % (m - 1))
            return plan
        return OpeningPlan(plan, self.in_domain, m, ROUNDS_LIMITS)

    def quotient_rounds(self, commitments, plan, values, lam, launches=None):
        """the DEEP quotient codeword (XArray) of a plan over the columns of several commitments: bfsr_deep_quotient_rounds, as many
        launches as the plan needs into one output.  values[g][j][r]: limb triples; launches: a ctypes.c_uint32 that receives their number"""
        return self._quotient(_lib.load().bfsr_deep_quotient_rounds, self._plan_arguments, commitments, plan, values, lam,
                              tail=(ctypes.byref(launches) if launches is not None else None,))

    def open_rounds(self, commitments, plan, proof_stream):
        """proves values of the polynomials of 1 .. 4 commitments of this PolynomialCommitment -- made at any moments of the same
        transcript -- under ONE plan, one quotient and one low-degree test.  The plan's columns are the row columns of all commitments
        numbered through (`global_column`); a group may hold columns of different commitments.  Returns values[g][j][r].  The plan is
        checked before any GPU work (ValueError)."""
        commitments = list(commitments)
        widths = self._widths([len(committed.polys) for committed in commitments])
        plan = self.rounds_plan(plan, widths)
        return self._open(commitments, plan, [(tuple(widths), plan.shape)], self.quotient_rounds, proof_stream)

    @_reads_leaf_pickles
    def verify_rounds(self, roots, widths, plan, values, proof_stream):
        """does the proof in `proof_stream` (read position where `open_rounds` began to push) show that the polynomials behind `roots`
        -- commitments of row widths `widths`, in the order `open_rounds` was given them -- take `values` (values[g][j][r]) under
        `plan`?  The roots are the caller's: it has read each from the transcript where `commit` pushed it.  Host code only; one printed
        line per refusal."""
        checked = self._checked_rounds(roots, widths, plan)
        return checked is not None and self._verify_plan(*checked, values, proof_stream)

    def _checked_rounds(self, roots, widths, plan):
        """(trees, plan, shape) as _verify_plan takes them for commitments of these roots and widths, or None with one printed line"""
        try:
            roots = list(roots)
            widths = self._widths(widths)
            if len(roots) != len(widths) or not all(isinstance(root, (bytes, bytearray)) for root in roots):
                raise ValueError("one root and one width per commitment (got %d and %d)" % (len(roots), len(widths)))
        except (TypeError, ValueError) as e:
            print("commitments cannot be opened: %s" % e)
            return None
        try:
            plan = self.rounds_plan(plan, widths)
        except ValueError as e:
            print("plan cannot be opened: %s" % e)
            return None
        return list(zip(roots, widths)), plan, (tuple(widths), plan.shape)

    @_reads_leaf_pickles
    def read_rounds(self, roots, widths, plan, proof_stream):
        """`verify_rounds` for a caller that does not know the values beforehand (a verifier that has drawn the points itself and wants
        the committed polynomials' values there): points and shape are checked against the caller's plan, the values are TAKEN from the
        stream and the quotient is checked against them.  Returns values[g][j][r] as limb triples -- exactly what an accepted opening
        vouches for -- or None on refusal, with one printed line.  Host code only."""
        checked = self._checked_rounds(roots, widths, plan)
        return None if checked is None else self._verify_plan(*checked, None, proof_stream, read=True)
