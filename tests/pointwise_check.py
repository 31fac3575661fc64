"""An independent check of the prover's pointwise stage: the AIR quotient codewords, the permutation-argument difference quotients
and the non-linear combination (brainfuck_stark.py:203-300 of the reference), recomputed in Python integers from the committed
codewords and compared word for word.

Two halves pin a codeword completely:
  * pointwise: on sampled rows every quotient and the combination are recomputed the way BrainfuckStark.verify does
    (brainfuck_stark.py ~940-975), except that the constraints are evaluated through Table.evaluate_constraints -- air.evaluate walking
    the expression graphs in Python, not the generated straight-line code the kernels run -- and the inner product is taken in Python;
  * degree: over the whole domain, the oracle's C INTT of the values.  On the coset offset * <omega> an INTT gives the coefficients
    times offset^k, so the zero pattern and with it the degree are those of the polynomial.  A few bad points break the degree bound;
    a systematic error of degree <= d agrees with the right polynomial on at most d of the n >= 4 d points, and each random row
    catches it with probability >= 3/4.
Every word of every buffer must also be a canonical residue (< p): a value v + p is the same field element and passes both halves.

Used by tests/test_gpu_prover_pointwise.py on buffers read back from the GPU and by tests/test_pointwise_checker.py on synthetic
codewords made with the oracle.  Nothing here calls the product's native code."""
import random
from hashlib import blake2b

import numpy as np

from oracle import ref_oracle as oracle
from stark_brainfuck_amd import air
from stark_brainfuck_amd.air import xadd, xmul, xscale, xsub

P = air.P
_P64 = np.uint64(P)
_EPSILON = np.uint64(0xFFFFFFFF)          # 2^64 = 2^32 - 1 (mod p)


def noncanonical(words):
    """flat positions of the words >= p"""
    return np.flatnonzero(np.asarray(words, dtype=np.uint64).reshape(-1) >= _P64)


def _add_mod(a, b):
    """a + b mod p for canonical uint64 arrays"""
    s = a + b
    s[s < b] += _EPSILON                   # the sum wrapped past 2^64: add 2^64 mod p (cannot wrap again)
    s[s >= _P64] -= _P64
    return s


def degree(planes, omega, seed=0):
    """degree of the polynomial whose values on a coset of <omega> are `planes` (n,) -- or the largest degree among the rows of a
    (k, n) array, folded into one codeword by a random linear combination with weights in [1, p) so that one INTT does (a degree the
    fold hides has probability < k / p).  -1 for the zero polynomial.  The values must be canonical."""
    planes = np.asarray(planes, dtype=np.uint64)
    planes = planes.reshape(-1, planes.shape[-1])
    n = planes.shape[1]
    if len(planes) == 1:
        folded = planes[0]
    else:
        rng = random.Random(seed)
        folded = np.zeros(n, dtype=np.uint64)
        for row in planes:
            folded = _add_mod(folded, oracle.hadamard(row, np.full(n, rng.randrange(1, P), dtype=np.uint64)))
    nonzero = np.flatnonzero(oracle.intt(omega, folded))
    return int(nonzero[-1]) if nonzero.size else -1


def sample_rows(n, unit_distances, count=1024, seed=0):
    """the rows the pointwise check looks at: both ends and the middle of the domain, the rows where a neighbour at unit distance u
    wraps around (u - 1, u, n - u - 1, n - u, n - u + 1), the powers of two from 2^8 on (block and grid-stride edges) and their
    neighbours, and `count` distinct uniform rows"""
    rows = {0, 1, 2, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1}
    for u in unit_distances:
        rows |= {u - 1, u, n - u - 1, n - u, n - u + 1}
    for k in range(8, n.bit_length() - 1):
        rows |= {(1 << k) - 1, 1 << k, (1 << k) + 1}
    rows |= set(random.Random(seed).sample(range(n), min(count, n)))
    return sorted({r % n for r in rows})


def sample_weights(number, seed):
    """the combination's weights (brainfuck_stark.py:104-112): weight i = ExtensionField.sample(blake2b(seed + bytes(i)).digest()),
    the three 21-byte big-endian chunks of the first 63 bytes, each mod p"""
    out, mask = [], (1 << 168) - 1
    for i in range(number):
        v = int.from_bytes(blake2b(bytes(seed) + bytes(i)).digest()[:63], "big")
        out.append(((v >> 336) % P, ((v >> 168) & mask) % P, (v & mask) % P))
    return out


def _inverse(v):
    return pow(v % P, P - 2, P)


class PointwiseSpec:
    """what the quotients and the combination of one proof are at a row, as functions of the committed codewords' values there.
    stark: the BrainfuckStark after prove() (tables padded, heights and lengths set); shift_tweak: the prover's test hook, applied to
    the array of degree shifts as the prover applies it."""

    def __init__(self, stark, challenges, terminals, quotient_degree_bounds, weights_seed, shift_tweak=None):
        self.tables, self.arguments = stark.tables, stark.permutation_arguments
        domain = stark.fri.domain
        self.n, self.offset, self.omega = domain.length, domain.offset.value, domain.omega.value
        self.max_degree = stark.max_degree
        self.challenges = tuple(tuple(int(v) for v in c) for c in challenges)
        self.terminals = tuple(tuple(int(v) for v in t) for t in terminals)
        self.labels = []                  # per quotient, in the prover's order: (table, kind, index within the kind)
        for t in self.tables:
            for kind, constraints in t.air.all():
                self.labels += [(type(t).__name__, kind, q) for q in range(len(constraints))]
        self.labels += [("permutation argument %d" % a, "difference", 0) for a in range(len(self.arguments))]
        assert len(quotient_degree_bounds) == len(self.labels)
        self.quotient_degree_bounds = list(quotient_degree_bounds)
        bounds = [t.interpolant_degree() for t in self.tables for _ in range(t.base_width)]
        bounds += [t.interpolant_degree() for t in self.tables for _ in range(t.full_width - t.base_width)]
        bounds += self.quotient_degree_bounds
        shifts = np.array([self.max_degree - b for b in bounds], dtype=np.uint64)
        if shift_tweak is not None:
            shifts = shift_tweak(shifts)
        self.shifts = [int(s) for s in shifts]
        self.weights = sample_weights(1 + 2 * len(bounds), weights_seed)

    def unit_distances(self):
        return sorted(set(t.unit_distance(self.n) for t in self.tables))

    def point(self, i):
        return self.offset * pow(self.omega, i, P) % P

    def quotients_at(self, i, values):
        """every quotient at row i, in the prover's order.  values(k, row): table k's base columns (lifted) then its extension
        columns at that row, as triples."""
        x = self.point(i)
        boundary = _inverse(x - 1)
        out = []
        for k, t in enumerate(self.tables):
            cur, nxt = values(k, i), values(k, (i + t.unit_distance(self.n)) % self.n)
            omicron_inverse = _inverse(t.omicron.value)
            zerofier = {"boundary": boundary,
                        "transition": 0 if t.height == 0 else (x - omicron_inverse) * _inverse(pow(x, t.height, P) - 1) % P,
                        "terminal": _inverse(x - omicron_inverse)}
            for kind, _ in t.air.all():
                out += [xscale(v, zerofier[kind]) for v in t.evaluate_constraints(kind, cur, nxt, self.challenges, self.terminals)]
        for arg in self.arguments:
            out.append(xscale(xsub(values(arg.lhs[0], i)[arg.lhs[1]], values(arg.rhs[0], i)[arg.rhs[1]]), boundary))
        return out

    def combination_at(self, i, values, randomizer, quotients):
        """w0 * randomizer + sum over the terms s of wa_s v_s + wb_s x^shift_s v_s, the terms in the reference's order: base columns of
        all tables, extension columns of all tables, quotients"""
        x = self.point(i)
        columns = [values(k, i) for k in range(len(self.tables))]
        terms = [v for t, c in zip(self.tables, columns) for v in c[:t.base_width]]
        terms += [v for t, c in zip(self.tables, columns) for v in c[t.base_width:]]
        terms += list(quotients)
        assert len(terms) == len(self.shifts)
        acc, powers = xmul(self.weights[0], randomizer), {}
        for s, (v, shift) in enumerate(zip(terms, self.shifts)):
            if shift not in powers:
                powers[shift] = pow(x, shift, P)
            acc = xadd(acc, xmul(self.weights[1 + 2 * s], v))
            acc = xadd(acc, xmul(self.weights[2 + 2 * s], xscale(v, powers[shift])))
        return acc


def _first(positions, n, limit=4):
    return ", ".join("row %d (plane %d)" % (p % n, p // n) for p in positions[:limit])


class Checker:
    """the checks of one proof's pointwise stage against host copies of its codewords.
    base[k]: (base_width, n) and ext[k]: (extension width, 3, n) of table k; randomizer: (3, n).  Each method returns a list of
    (kind, message) failures, kind one of "canonical", "pointwise", "degree"."""

    def __init__(self, spec, base, ext, randomizer, rows):
        self.spec, self.base, self.ext, self.randomizer, self.rows = spec, base, ext, randomizer, list(rows)
        n = spec.n
        # the values the expected quotients read: the rows and their neighbours at every table's unit distance
        needed = set(self.rows) | {(i + t.unit_distance(n)) % n for i in self.rows for t in spec.tables}
        needed = sorted(needed)
        at = {r: c for c, r in enumerate(needed)}
        cols = np.array(needed, dtype=np.int64)
        picked = [(b[:, cols], e[:, :, cols]) for b, e in zip(base, ext)]

        def values(k, row):
            b, e = picked[k]
            c = at[row]
            return [(int(v), 0, 0) for v in b[:, c]] + [tuple(int(v) for v in e[m, :, c]) for m in range(e.shape[0])]
        self.values = values
        self.expected = {i: spec.quotients_at(i, values) for i in self.rows}
        self.index = np.array(self.rows, dtype=np.int64)

    def inputs(self, degrees=True):
        """the codewords the stage reads: canonical; with degrees, the extension codewords of degree <= the table's interpolant
        degree (one INTT per table) and the randomizer codeword <= max_degree"""
        spec, n, out = self.spec, self.spec.n, []
        for t, b, e in zip(spec.tables, self.base, self.ext):
            name = type(t).__name__
            for what, words in (("base", b), ("extension", e)):
                bad = noncanonical(words)
                if bad.size:
                    out.append(("canonical", "%s %s codewords: %d words >= p, at %s" % (name, what, bad.size, _first(bad, n))))
        bad = noncanonical(self.randomizer)
        if bad.size:
            out.append(("canonical", "randomizer codeword: %d words >= p, at %s" % (bad.size, _first(bad, n))))
        if degrees and not out:
            for t, e in zip(spec.tables, self.ext):
                if e.size:
                    d = degree(e.reshape(-1, n), spec.omega)
                    if d > t.interpolant_degree():
                        out.append(("degree", "%s extension codewords: degree %d > %d" % (type(t).__name__, d, t.interpolant_degree())))
            d = degree(self.randomizer, spec.omega)
            if d > spec.max_degree:
                out.append(("degree", "randomizer codeword: degree %d > max_degree %d" % (d, spec.max_degree)))
        return out

    def quotient(self, q, codeword, check_degree=True):
        """quotient q of the prover's list, (3, n): canonical, the expected values on the sampled rows, degree <= its bound"""
        spec, n = self.spec, self.spec.n
        table, kind, index = spec.labels[q]
        label = "%s %s quotient %d" % (table, kind, index)
        codeword = np.asarray(codeword, dtype=np.uint64).reshape(3, n)
        bad = noncanonical(codeword)
        if bad.size:
            return [("canonical", "%s: %d words >= p, at %s" % (label, bad.size, _first(bad, n)))]
        out = []
        want = np.array([self.expected[i][q] for i in self.rows], dtype=np.uint64).T
        wrong = np.flatnonzero((codeword[:, self.index] != want).any(axis=0))
        if wrong.size:
            i = self.rows[wrong[0]]
            out.append(("pointwise", "%s differs at %d of %d sampled rows, first at row %d: %s, expected %s" % (
                label, wrong.size, len(self.rows), i, tuple(int(v) for v in codeword[:, i]), self.expected[i][q])))
        if check_degree:
            d, bound = degree(codeword, spec.omega), spec.quotient_degree_bounds[q]
            if d > max(bound, -1):                  # (the zero polynomial meets every bound, a negative one of an empty table too)
                out.append(("degree", "%s: degree %d > bound %d" % (label, d, bound)))
        return out

    def combination(self, codeword, check_degree=True):
        """the combination codeword, (3, n): canonical, the expected values on the sampled rows, degree <= max_degree"""
        spec, n = self.spec, self.spec.n
        codeword = np.asarray(codeword, dtype=np.uint64).reshape(3, n)
        bad = noncanonical(codeword)
        if bad.size:
            return [("canonical", "combination: %d words >= p, at %s" % (bad.size, _first(bad, n)))]
        out = []
        rand = self.randomizer[:, self.index]
        want = np.array([spec.combination_at(i, self.values, tuple(int(v) for v in rand[:, c]), self.expected[i])
                         for c, i in enumerate(self.rows)], dtype=np.uint64).T
        wrong = np.flatnonzero((codeword[:, self.index] != want).any(axis=0))
        if wrong.size:
            c = wrong[0]
            out.append(("pointwise", "combination differs at %d of %d sampled rows, first at row %d: %s, expected %s" % (
                wrong.size, len(self.rows), self.rows[c], tuple(int(v) for v in codeword[:, self.rows[c]]),
                tuple(int(v) for v in want[:, c]))))
        if check_degree:
            d = degree(codeword, spec.omega)
            if d > spec.max_degree:
                out.append(("degree", "combination: degree %d > max_degree %d" % (d, spec.max_degree)))
        return out
