"""tests/subproduct_check.py checked without a GPU: its checkers accept the Lagrange interpolant and the product of linear factors
computed on Python integers, refuse every single-word change of them and every wrong length; its domains are what they say; and
the sizes the GPU tests run reach every node shape and every branch of the long evaluation (the floor)."""
import numpy as np
import pytest

import subproduct_check as sc

P = sc.P
SIZES = [1, 2, 5, 129, 133]
FREE = {1: (), 2: (0,), 5: sc.FREE_POINTS[:3], 129: sc.FREE_POINTS, 133: ()}


def product_of_factors(pts):
    z = [1]
    for x in pts:
        nz = [0] * (len(z) + 1)
        for i, c in enumerate(z):
            nz[i + 1] = (nz[i + 1] + c) % P
            nz[i] = (nz[i] - c * x) % P
        z = nz
    return z


def lagrange(pts, values):
    """the interpolant's n coefficients: sum_i v_i / Z'(x_i) * Z / (X - x_i), the quotients by synthetic division"""
    n = len(pts)
    z = product_of_factors(pts)
    out = [0] * n
    for x, v in zip(pts, values):
        q, acc = [0] * n, 0
        for i in range(n, 0, -1):
            acc = (z[i] + acc * x) % P
            q[i - 1] = acc
        w = v * pow(sc.horner(q, x), P - 2, P) % P
        for i in range(n):
            out[i] = (out[i] + w * q[i]) % P
    return out


@pytest.fixture(scope="module", params=SIZES)
def case(request):
    n = request.param
    dom = sc.ragged(n, 5, FREE[n])
    pts = [int(v) for v in sc.points(dom)]
    values = sc.column("random", n, 100 + n)
    coeffs = sc.column("random", n + 3, 200 + n)
    return dict(n=n, dom=dom, pts=pts, values=values, coeffs=coeffs,
                interpolant=np.array(lagrange(pts, [int(v) for v in values]), dtype=np.uint64),
                zerofier=np.array(product_of_factors(pts), dtype=np.uint64),
                evaluation=np.array([sc.horner([int(c) for c in coeffs], x) for x in pts], dtype=np.uint64))


def changed(vec, i):
    out = vec.copy()
    out[i] = (int(out[i]) + 1) % P
    return out


def refused(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def test_integer_results_are_accepted(case):
    sc.check_interpolant(case["dom"], case["values"], case["interpolant"])
    sc.check_zerofier(case["dom"], case["zerofier"])
    sc.check_evaluate(case["dom"], case["coeffs"], case["evaluation"])
    assert (sc.evaluate_everywhere(case["dom"], case["coeffs"]) == case["evaluation"]).all()
    for m in (0, 1, 2, case["n"], 4 * case["n"] + 1):                      # every transform size of the reference against Horner
        coeffs = sc.column("palette", m, 0)
        want = [sc.horner([int(c) for c in coeffs], x) for x in case["pts"]]
        assert sc.evaluate_everywhere(case["dom"], coeffs).tolist() == want, m


def test_every_single_word_change_is_refused(case):
    n, dom = case["n"], case["dom"]
    assert all(refused(sc.check_interpolant, dom, case["values"], changed(case["interpolant"], i)) for i in range(n))
    assert all(refused(sc.check_zerofier, dom, changed(case["zerofier"], i)) for i in range(n + 1))
    assert all(refused(sc.check_evaluate, dom, case["coeffs"], changed(case["evaluation"], i)) for i in range(n))
    assert all(refused(sc.check_interpolant, dom, changed(case["values"], i), case["interpolant"]) for i in range(n))


def test_wrong_lengths_and_residues_are_refused(case):
    n, dom = case["n"], case["dom"]
    zero = np.zeros(1, dtype=np.uint64)
    for check, args, good in ((sc.check_interpolant, (dom, case["values"]), case["interpolant"]),
                              (sc.check_zerofier, (dom,), case["zerofier"]),
                              (sc.check_evaluate, (dom, case["coeffs"]), case["evaluation"])):
        assert refused(check, *args, good[:-1])
        assert refused(check, *args, np.concatenate([good, zero]))         # a longer vector with the same polynomial
        assert refused(check, *args, good.reshape(1, -1))
        high = good.copy()
        high[-1] = np.uint64(0xFFFFFFFFDEADBEEF)                             # the paint of tests/painted.py: no residue
        assert refused(check, *args, high)


def test_the_assertion_names_the_first_differing_position(case):
    n, dom = case["n"], case["dom"]
    i = n // 2
    with pytest.raises(AssertionError, match="position %d of %d " % (i, n)):
        sc.check_evaluate(dom, case["coeffs"], changed(case["evaluation"], i))
    with pytest.raises(AssertionError, match="at position %d it takes" % i):
        sc.check_interpolant(dom, changed(case["values"], i), case["interpolant"])


@pytest.mark.parametrize("n", SIZES + [257, 4100])
def test_domains_are_seeded_distinct_and_hold_the_free_points(n):
    free = FREE.get(n, sc.FREE_POINTS)
    a, b, c = sc.ragged(n, 3, free), sc.ragged(n, 3, free), sc.ragged(n, 4, free)
    pa = sc.points(a)
    assert (pa == sc.points(b)).all() and a.entries == b.entries
    assert n <= 2 or a.entries != c.entries
    assert pa.size == n and len(set(pa.tolist())) == n and (pa < np.uint64(P)).all()
    assert [int(pa[p]) for p in sc.free_positions(n, len(free))] == list(free)
    if n > 128 and len(free) == len(sc.FREE_POINTS):
        last = ((n - 1) >> 7) << 7
        assert set(sc.free_positions(n, len(free))) >= {0, n - 1, 127, 128, last}
    M = max(1 << sc.log2_ceil(n), 2)
    for g in a.groups:                                                       # every point is what its descriptor says
        if g[0] == "coset":
            assert g[1] in sc.OFFSETS and g[2] == M
    w = sc.oracle.primitive_nth_root(M)
    for pos, e in enumerate(a.entries[:40]):
        assert int(pa[pos]) == (e[1] if e[0] == "free" else e[1] * pow(w, e[3], P) % P)
    eq = sc.with_equal(a, [(0, n - 1)])
    pe = sc.points(eq)
    assert pe[0] == pe[n - 1] == pa[0] and (pe[1:n - 1] == pa[1:n - 1]).all()


@pytest.mark.parametrize("k,r", [(3, 1), (8, 4)])
def test_table_shape_is_the_reference_call(k, r):
    dom = sc.table_shape(k, r)
    order = dom.order
    assert order == 8 << k and len(dom) == (1 << k) + r and len(dom.groups) == 2
    omicron, w = sc.oracle.primitive_nth_root(1 << k), sc.oracle.primitive_nth_root(order)
    want = [pow(omicron, i, P) for i in range(1 << k)] + [pow(w, 2 * i + 1, P) for i in range(r)]
    assert sc.points(dom).tolist() == want
    sc.check_zerofier(dom, np.array(product_of_factors(want), dtype=np.uint64))


def test_column_kinds():
    for kind in sc.KINDS:
        col = sc.column(kind, 40, 9)
        assert col.dtype == np.uint64 and col.size == 40 and (col < np.uint64(P)).all()
        assert sc.column(kind, 0, 9).size == 0
    assert not sc.column("zero", 40, 9).any() and (sc.column("pm1", 40, 9) == np.uint64(P - 1)).all()
    first, last = sc.column("first", 40, 9), sc.column("last", 40, 9)
    assert first[0] and not first[1:].any() and last[-1] and not last[:-1].any()
    assert sc.column("palette", 40, 9)[:15].tolist() == list(sc.field_states.PALETTE)
    seven = sc.columns(7, 40, 9)
    assert seven.shape == (7, 40) and (seven[0] != seven[6]).any() and set(sc.BATCH_KINDS[7]) == set(sc.KINDS)


# ------------------------------------------------------------------------------------------------ the floor
def test_restated_degrees():
    for n in (129, 256, 257, 1000):
        L = sc.log2_ceil(n)
        for k in range(L + 1):
            degs = [sc.node_deg(n, k, c) for c in range(1 << (L - k))]
            assert sum(degs) == n and all(0 <= d <= 1 << k for d in degs)
            assert all(a == 1 << k or b == 0 for a, b in zip(degs, degs[1:]))          # full nodes, at most one partial, then empty


def test_tree_sizes_reach_every_shape():
    reached = set()
    for n in sc.TREE_SIZES:
        reached |= sc.shape_classes(n)
    assert sc.SHAPE_REQUIRED <= reached, sorted(sc.SHAPE_REQUIRED - reached)
    assert not reached & set(sc.SHAPE_EXCLUDED)
    for n in range(129, 1200):                                               # the exclusions are the arithmetic's, not the list's
        assert not sc.shape_classes(n) & set(sc.SHAPE_EXCLUDED), n
    assert set(sc.FREE_SIZES) <= set(sc.TREE_SIZES)


def test_coefficient_counts_reach_every_long_branch():
    reached = {sc.long_classes(n, m) for n, m in sc.long_cases()}
    assert sc.LONG_REQUIRED <= reached, sorted(sc.LONG_REQUIRED - reached)
    assert all(reason for reason in sc.LONG_EXCLUDED.values()) and not reached & set(sc.LONG_EXCLUDED)
    for n in range(1, 70):
        for m in range(n + 1, 6 * n + 140):
            assert sc.long_classes(n, m) not in sc.LONG_EXCLUDED, (n, m)
    # the l1 > l2 branch is the small trees', and the large trees take both stagings of the quotient
    assert any(sc.long_classes(n, m)[2] == "l1>l2" for n, m in sc.long_cases() if n in sc.SMALL_SIZES)
    for n in sc.TREE_SIZES:
        counts = sc.coefficient_counts(n)
        assert {1, 2, n - 1, n, n + 1, n + 2, n + 128, n + 129} <= set(counts)
        assert {sc.long_classes(n, m)[1] for m in counts if m > n} == {"s2<=N", "s2>N"} or n & (n - 1) == 0
