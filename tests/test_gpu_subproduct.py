"""The subproduct tree on the MI355X (csrc/subproduct.hip, SubproductTree, the array and list forms of fast_zerofier /
fast_evaluate / fast_interpolate): against the reference's fixtures, the private recursion, host arithmetic on Python ints and the
NTT on cosets; and, on ragged domains whose trees have partial and empty nodes, at EVERY output against the oracle's coset
transform (tests/subproduct_check.py).  Expected values never come from the tree itself."""
import ctypes
import importlib
import random

import numpy as np
import pytest

import subproduct_check as sc
from conftest import load_golden
from painted import PAINT_WORD, Arena
from stream_builders import strided

pytestmark = pytest.mark.gpu

P = (1 << 64) - (1 << 32) + 1


@pytest.fixture(scope="module")
def sb():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    import stark_brainfuck_amd
    return stark_brainfuck_amd


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % P
    return acc


def zerofier_at(points, r):
    acc = 1
    for x in points:
        acc = acc * (r - x) % P
    return acc


def rand_points(rng, n):
    pts = set()
    while len(pts) < n:
        pts.add(rng.randrange(P))
    out = list(pts)
    rng.shuffle(out)
    return out


def rand_vec(rng, n):
    return [rng.randrange(P) for _ in range(n)]


def base_array(sb, rows):
    return sb.BaseArray.from_numpy(np.array(rows, dtype=np.uint64))


def x_array(sb, limbs):
    return sb.XArray.from_numpy(np.array(limbs, dtype=np.uint64))


# ---- reference fixtures -------------------------------------------------------------------------------------------------------------

def test_poly2_fixtures_through_the_tree(sb):
    F = sb.BaseField.main()
    for c in load_golden("poly2.json")["cases"]:
        n = c["N"]
        tree = sb.SubproductTree([F(v) for v in c["domain"]])
        assert tree.zerofier().to_numpy().tolist() == c["zerofier"]
        assert tree.interpolate(base_array(sb, c["values"])).to_numpy().reshape(-1).tolist()[:len(c["interpolant"])] == c["interpolant"]
        assert tree.evaluate(base_array(sb, c["poly"])).to_numpy().reshape(-1).tolist() == c["poly_evaluated"]
        interp = base_array(sb, c["interpolant"])
        assert tree.evaluate(interp).to_numpy().reshape(-1).tolist() == c["values"]
        # the array forms of the public functions
        w = F.primitive_nth_root(c["root_order"])
        D = base_array(sb, c["domain"])
        assert sb.fast_zerofier(D, w, c["root_order"]).to_numpy().tolist() == c["zerofier"]
        coeffs = sb.fast_interpolate(D, base_array(sb, c["values"]), w, c["root_order"])
        assert isinstance(coeffs, sb.BaseArray) and len(coeffs) == n
        assert coeffs.to_numpy().reshape(-1).tolist()[:len(c["interpolant"])] == c["interpolant"]
        vals = sb.fast_evaluate(base_array(sb, c["poly"]), D, w, c["root_order"])
        assert isinstance(vals, sb.BaseArray) and vals.to_numpy().reshape(-1).tolist() == c["poly_evaluated"]


def test_polyx_interpolate_columns_fixtures_through_the_tree(sb):
    g = load_golden("polyx.json")
    for c in g["interpolate_columns"]:
        if any(l[1] or l[2] for l in c["domain"]):
            continue
        pts = [l[0] for l in c["domain"]]
        tree = sb.SubproductTree(base_array(sb, pts))
        assert [[v, 0, 0] for v in tree.zerofier().to_numpy().tolist()] == c["zerofier"]
        vals = x_array(sb, np.array(c["values"], dtype=np.uint64).T)
        poly = tree.interpolate(vals)
        assert isinstance(poly, sb.XArray)
        got = poly.to_numpy().T.tolist()
        assert got[:len(c["interpolant"])] == c["interpolant"]
        assert all(r == [0, 0, 0] for r in got[len(c["interpolant"]):])
        assert tree.evaluate(poly).to_numpy().T.tolist() == c["values"]


# ---- arbitrary domains ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 64, 65, 127, 1000, 1024, 4097])
def test_arbitrary_domains_against_host_arithmetic(sb, n):
    rng = random.Random(1000 + n)
    pts = rand_points(rng, n)
    tree = sb.SubproductTree(base_array(sb, pts))
    samples = list(range(n)) if n <= 128 else rng.sample(range(n), 24)
    # zerofier: monic of degree n, vanishing on the domain, equal to the product of linear factors elsewhere
    z = tree.zerofier().to_numpy().tolist()
    assert len(z) == n + 1 and z[-1] == 1
    for i in samples[:8]:
        assert horner(z, pts[i]) == 0
    for r in rand_vec(rng, 4):
        assert horner(z, r) == zerofier_at(pts, r)
    # evaluation of 1 and 3 columns, degrees below, equal to and above n
    for m in sorted({max(n - 1, 1), n, n + 1, 2 * n + 5}):
        for cols in (1, 3):
            coeffs = [rand_vec(rng, m) for _ in range(cols)]
            out = tree.evaluate(base_array(sb, coeffs if cols > 1 else coeffs[0])).to_numpy().reshape(cols, n)
            for b in range(cols):
                for i in samples:
                    assert int(out[b, i]) == horner(coeffs[b], pts[i]), (m, b, i)
    # interpolation of 1 and 3 columns: the interpolant has n coefficients and takes the values
    for cols in (1, 3):
        values = [rand_vec(rng, n) for _ in range(cols)]
        out = tree.interpolate(base_array(sb, values if cols > 1 else values[0])).to_numpy().reshape(cols, n)
        for b in range(cols):
            poly = [int(v) for v in out[b]]
            for i in samples:
                assert horner(poly, pts[i]) == values[b][i]


@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 64, 65])
def test_small_domains_against_the_recursion(sb, n):
    ntt_mod = importlib.import_module("stark_brainfuck_amd.ntt")       # (the package attribute `ntt` is the function)
    F = sb.BaseField.main()
    rng = random.Random(n)
    order = 128
    w = F.primitive_nth_root(order)
    D = [F(v) for v in rand_points(rng, n)]
    V = [F(v) for v in rand_vec(rng, n)]
    poly = sb.Polynomial([F(v) for v in rand_vec(rng, n + 3)])
    tree = sb.SubproductTree(D)
    assert tree.zerofier().to_numpy().tolist() == [c.value for c in ntt_mod._fast_zerofier_recursive(D, w, order).coefficients]
    ref = ntt_mod._fast_interpolate_recursive(D, V, w, order)
    assert tree.interpolate(base_array(sb, [v.value for v in V])).to_numpy().tolist() == [c.value for c in ref.coefficients]
    got = tree.evaluate(base_array(sb, [c.value for c in poly.coefficients])).to_numpy().tolist()
    assert got == [v.value for v in ntt_mod._fast_evaluate_recursive(poly, D, w, order)]


def test_duplicate_points_raise(sb):
    tree = sb.SubproductTree(base_array(sb, [5, 7, 9, 7] + list(range(100, 200))))
    with pytest.raises(AssertionError):
        tree.interpolate(base_array(sb, list(range(104))))


# ---- full size against the NTT on cosets ---------------------------------------------------------------------------------------------

def _coset_ntt(sb, coeffs, shift, log_n):
    """p(shift * w^k), k < 2^log_n, of the 2^log_n coefficients `coeffs`: bfs_gl_ntt with a coset shift"""
    from stark_brainfuck_amd.arrays import raw_ntt
    n = 1 << log_n
    src = sb.BaseArray.from_numpy(np.asarray(coeffs, dtype=np.uint64))
    out = sb.BaseArray.empty(n)
    raw_ntt(src.ptr, len(coeffs), len(coeffs), out.ptr, n, log_n, 1, sb.BaseField.main().primitive_nth_root(n).value, shift)
    return out.to_numpy()


@pytest.mark.parametrize("log_n", [16, 18, 20])
def test_union_of_cosets_against_the_ntt(sb, log_n):
    """the domain is a shuffled union of 4 cosets c_k <w>, |<w>| = n / 4: c_k <w> is every 4th point of c_k <w_n>, on which the NTT of
    size n evaluates a polynomial of n coefficients"""
    n, m = 1 << log_n, 1 << (log_n - 2)
    rng = np.random.default_rng(log_n)
    offsets = [7, pow(7, 3, P), pow(7, 5, P), pow(7, 11, P)]
    e1 = np.zeros(n, dtype=np.uint64)
    e1[1] = 1
    pts = np.concatenate([_coset_ntt(sb, e1, c, log_n)[::4] for c in offsets])       # c w_n^(4j) = c w^j
    perm = rng.permutation(n)
    dom = pts[perm]
    where = np.empty(n, dtype=np.int64)
    where[perm] = np.arange(n)                  # where[j] = position in `dom` of point j of the union
    tree = sb.SubproductTree(sb.BaseArray.from_numpy(dom))
    coeffs = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
    ev = tree.evaluate(sb.BaseArray.from_numpy(coeffs)).to_numpy()
    for k, c in enumerate(offsets):
        assert (ev[where[k * m:(k + 1) * m]] == _coset_ntt(sb, coeffs, c, log_n)[::4]).all(), k
    values = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
    poly = tree.interpolate(sb.BaseArray.from_numpy(values)).to_numpy()
    for k, c in enumerate(offsets):
        assert (_coset_ntt(sb, poly, c, log_n)[::4] == values[where[k * m:(k + 1) * m]]).all(), k
    z = [int(v) for v in tree.zerofier().to_numpy()]
    assert len(z) == n + 1 and z[-1] == 1
    pr = random.Random(log_n)
    dl = [int(v) for v in dom]
    for _ in range(8):
        r = pr.randrange(P)
        assert horner(z, r) == zerofier_at(dl, r)


# ---- batching -------------------------------------------------------------------------------------------------------------------

def test_columns_equal_single_calls(sb):
    rng = random.Random(8)
    n = 3000
    tree = sb.SubproductTree(base_array(sb, rand_points(rng, n)))
    cols = [rand_vec(rng, n) for _ in range(8)]
    many = tree.interpolate(base_array(sb, cols)).to_numpy()
    ev = tree.evaluate(base_array(sb, cols)).to_numpy()
    for b in range(8):
        assert (many[b] == tree.interpolate(base_array(sb, cols[b])).to_numpy()).all()
        assert (ev[b] == tree.evaluate(base_array(sb, cols[b])).to_numpy()).all()
    xv = x_array(sb, cols[:3])
    xi, xe = tree.interpolate(xv).to_numpy(), tree.evaluate(xv).to_numpy()
    for k in range(3):
        assert (xi[k] == many[k]).all() and (xe[k] == ev[k]).all()


# ---- list path parity ---------------------------------------------------------------------------------------------------------------

def _same(a, b):
    return len(a) == len(b) and all(type(x) is type(y) and x == y for x, y in zip(a, b))


def _call(fn, *args):
    try:
        return ("ok", fn(*args))
    except Exception as e:          # the routed call must fail exactly when the recursion does, with the same exception
        return ("err", type(e), str(e))


def _same_outcome(a, b):
    if a[0] != b[0]:
        return False
    if a[0] == "err":
        return a[1:] == b[1:]
    ra, rb = a[1], b[1]
    if isinstance(ra, list):
        return _same(ra, rb)
    return _same(ra.coefficients, rb.coefficients)


@pytest.mark.parametrize("dom_x", [False, True])
@pytest.mark.parametrize("val_x", [False, True])
@pytest.mark.parametrize("root_x", [False, True])
def test_list_calls_match_the_recursion(sb, dom_x, val_x, root_x):
    ntt_mod = importlib.import_module("stark_brainfuck_amd.ntt")       # (the package attribute `ntt` is the function)
    XF = sb.ExtensionField.main()
    F = XF._base()
    rng = random.Random(100 + 4 * dom_x + 2 * val_x + root_x)
    for n, order in ((100, 128), (128, 128)):
        w = F.primitive_nth_root(order)
        root = XF.lift(w) if root_x else w
        D = [F(v) for v in rand_points(rng, n)]
        if dom_x:
            D = [XF.lift(x) for x in D]
        V = [XF.from_limbs(rand_vec(rng, 3)) for _ in range(n)] if val_x else [F(v) for v in rand_vec(rng, n)]
        poly = sb.Polynomial(V + V[:7])
        assert _same_outcome(_call(sb.fast_zerofier, D, root, order), _call(ntt_mod._fast_zerofier_recursive, D, root, order))
        assert _same_outcome(_call(sb.fast_interpolate, D, V, root, order), _call(ntt_mod._fast_interpolate_recursive, D, V, root, order))
        assert _same_outcome(_call(sb.fast_evaluate, poly, D, root, order), _call(ntt_mod._fast_evaluate_recursive, poly, D, root, order))
    # two equal points: the recursion's own error
    D2 = D[:99] + D[:1]
    assert _same_outcome(_call(sb.fast_interpolate, D2, V[:100], root, 128),
                         _call(ntt_mod._fast_interpolate_recursive, D2, V[:100], root, 128))


def test_root_assertions_come_first(sb):
    F = sb.BaseField.main()
    D = [F(v) for v in range(100)]
    with pytest.raises(AssertionError, match="supplied root does not have supplied order"):
        sb.fast_interpolate(D, D, F(3), 128)
    with pytest.raises(AssertionError, match="supplied root is not primitive root of supplied order"):
        sb.fast_zerofier(D, F.primitive_nth_root(64), 128)


def test_lifted_memory_table_shape_is_fast(sb):
    """one Table.interpolate_columns column of a 4096-row table: lifted domain and root, extension values"""
    import time
    XF = sb.ExtensionField.main()
    F = XF._base()
    rng = random.Random(4096)
    n, order = 4096 + 4, 1 << 15
    omicron = F.primitive_nth_root(4096)
    D = [XF.lift(omicron ^ i) for i in range(4096)] + [XF.lift(F.primitive_nth_root(order) ^ (2 * i + 1)) for i in range(4)]
    V = [XF.from_limbs(rand_vec(rng, 3)) for _ in range(n)]
    root = XF.lift(F.primitive_nth_root(order))
    sb.fast_interpolate(D[:200], V[:200], root, order)           # warm-up (library, tables)
    t = time.perf_counter()
    poly = sb.fast_interpolate(D, V, root, order)
    dt = time.perf_counter() - t
    assert len(poly.coefficients) == n and all(type(c) is sb.ExtensionFieldElement for c in poly.coefficients)
    for i in rng.sample(range(n), 6):
        assert poly.evaluate(D[i]) == V[i]
    assert dt < 1.0, dt


# ---- every output, on domains with partial and empty nodes (tests/subproduct_check.py) -------------------------------------------------
# A domain is made of points the oracle's coset transform reaches (plus a few free points for Horner), so all n outputs of all
# three operations are decided on the CPU without O(n^2) work: an evaluation is compared word for word, an interpolant is the one
# vector of n words that takes the values, a zerofier the one monic vector of n + 1 words that vanishes on the domain.
# tests/test_subproduct_checker.py holds the checkers to that and the size lists to the node shapes they must reach.
BFS_ERR_ZERO_IN_BATCH_INVERSE = 5
SEED = 0x5B


@pytest.fixture(scope="module")
def lib(sb):
    from stark_brainfuck_amd import _lib
    return _lib.load()


def ok(rc):
    from stark_brainfuck_amd import _lib
    _lib.check(rc)


def ragged_domain(n):
    return sc.ragged(n, SEED, sc.FREE_POINTS if n in sc.FREE_SIZES else ())


def tree_of(sb, dom):
    return sb.SubproductTree(sb.BaseArray.from_numpy(sc.points(dom)))


def check_all_three(sb, dom, tree, counts, seed):
    """zerofier, one evaluation per coefficient count and a three-column interpolation of `tree` through the checkers"""
    n = len(dom)
    sc.check_zerofier(dom, tree.zerofier().to_numpy())
    for m in counts:
        coeffs = sc.column("random", m, seed + m)
        sc.check_evaluate(dom, coeffs, tree.evaluate(sb.BaseArray.from_numpy(coeffs)).to_numpy())
    values = sc.columns(3, n, seed)
    got = tree.interpolate(sb.BaseArray.from_numpy(values)).to_numpy()
    assert got.shape == (3, n)
    for b in range(3):
        sc.check_interpolant(dom, values[b], got[b])


@pytest.mark.parametrize("n", sc.SMALL_SIZES + sc.TREE_SIZES)
def test_every_output_on_ragged_domains(sb, n):
    dom = ragged_domain(n)
    check_all_three(sb, dom, tree_of(sb, dom), sc.coefficient_counts(n), 31 * n)


class AbiTree:
    """bfs_ptree_build over a domain, freed on exit; `points` is the device copy the tree was built from"""

    def __init__(self, lib, dom):
        from stark_brainfuck_amd.device import DeviceBuffer
        self.lib, self.host = lib, sc.points(dom)
        self.points = DeviceBuffer.from_numpy(self.host)
        self.handle = ctypes.c_void_p()
        ok(lib.bfs_ptree_build(self.points.ptr, len(dom), 0, ctypes.byref(self.handle)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        from stark_brainfuck_amd.device import synchronize
        ok(self.lib.bfs_ptree_free(self.handle, 0))
        synchronize(0)


def strided_input(cols, stride):
    """the columns `stride` apart on the device, the gaps numbered; (device buffer, host copy)"""
    from stark_brainfuck_amd.device import DeviceBuffer
    host = strided(cols, stride, np.arange(1, cols.shape[0] * stride + 1, dtype=np.uint64))
    return DeviceBuffer.from_numpy(host), host


@pytest.mark.parametrize("batch", [1, 3, 7])
@pytest.mark.parametrize("n", [257, 4100])
def test_strided_columns_of_every_kind_through_the_c_abi(lib, n, batch):
    """in_stride = m + 5, out_stride = n + 3: every column against the checker, the words between the columns of the output and
    around it keep their paint, inputs and points read back as they went up; no coefficients at all give zeros"""
    dom = ragged_domain(n)
    out_stride = n + 3
    with AbiTree(lib, dom) as tree:
        assert lib.bfs_ptree_size(tree.handle) == n
        for m in (0, 1, n, n + 129, 2 * n + 5):
            in_stride = m + 5
            cols = sc.columns(batch, m, SEED + m)
            src, host = strided_input(cols, in_stride)
            out = Arena(batch=batch, stride=out_stride, n=n)
            ok(lib.bfs_ptree_evaluate(tree.handle, src.ptr if m else None, m, in_stride, batch, out.ptr, out_stride, 0))
            got = out.rows(out.contained([("coefficients", host, src.to_numpy()), ("points", tree.host, tree.points.to_numpy())]))
            for b in range(batch):
                if m == 0:
                    assert not got[b].any(), b
                else:
                    sc.check_evaluate(dom, cols[b], got[b])
        in_stride = n + 5
        values = sc.columns(batch, n, SEED + 1)
        src, host = strided_input(values, in_stride)
        out = Arena(batch=batch, stride=out_stride, n=n)
        ok(lib.bfs_ptree_interpolate(tree.handle, src.ptr, in_stride, batch, out.ptr, out_stride, 0))
        got = out.rows(out.contained([("values", host, src.to_numpy()), ("points", tree.host, tree.points.to_numpy())]))
        for b in range(batch):
            sc.check_interpolant(dom, values[b], got[b])


@pytest.mark.parametrize("n", [385, 4100])
def test_extension_columns_limb_by_limb(sb, n):
    dom = ragged_domain(n)
    tree = tree_of(sb, dom)
    for m in (n - 1, n + 129):
        limbs = sc.columns(3, m, SEED + 2 * m)
        got = tree.evaluate(sb.XArray.from_numpy(limbs))
        assert isinstance(got, sb.XArray)
        got = got.to_numpy()
        assert got.shape == (3, n)
        for k in range(3):
            sc.check_evaluate(dom, limbs[k], got[k])
    values = sc.columns(3, n, SEED + 3)
    got = tree.interpolate(sb.XArray.from_numpy(values))
    assert isinstance(got, sb.XArray)
    got = got.to_numpy()
    assert got.shape == (3, n)
    for k in range(3):
        sc.check_interpolant(dom, values[k], got[k])


def limb_planes(elements):
    """(3, len) limbs of a list of ExtensionFieldElements, read from the objects"""
    out = np.zeros((3, len(elements)), dtype=np.uint64)
    for i, e in enumerate(elements):
        for k, c in enumerate(e.polynomial.coefficients):
            out[k, i] = c.value
    return out


@pytest.mark.parametrize("r", [1, 4])
@pytest.mark.parametrize("k", [8, 12])
def test_table_shape_at_every_output(sb, k, r):
    """what Table.interpolate_columns passes: 2^k rows and r randomizer points -- one full half, a sibling of degree r and empty
    nodes all the way up.  Through SubproductTree, and through the list calls with lifted domain, lifted root, extension values."""
    dom = sc.table_shape(k, r)
    n, order = len(dom), dom.order
    check_all_three(sb, dom, tree_of(sb, dom), (n - 1, n, n + 1, 2 * n + 5), 77 * n)
    XF = sb.ExtensionField.main()
    F = XF._base()
    root = XF.lift(F.primitive_nth_root(order))
    D = [XF.lift(F(int(x))) for x in sc.points(dom)]
    z = sb.fast_zerofier(D, root, order)
    assert all(type(c) is sb.ExtensionFieldElement for c in z.coefficients)
    planes = limb_planes(z.coefficients)
    sc.check_zerofier(dom, planes[0])
    assert not planes[1:].any()
    values = sc.columns(3, n, 78 * n)
    poly = sb.fast_interpolate(D, [XF.from_limbs([int(v) for v in values[:, i]]) for i in range(n)], root, order)
    assert len(poly.coefficients) == n and all(type(c) is sb.ExtensionFieldElement for c in poly.coefficients)
    planes = limb_planes(poly.coefficients)
    for l in range(3):
        sc.check_interpolant(dom, values[l], planes[l])
    coeffs = sc.columns(3, n + 3, 79 * n)
    ev = sb.fast_evaluate(sb.Polynomial([XF.from_limbs([int(v) for v in coeffs[:, i]]) for i in range(n + 3)]), D, root, order)
    assert len(ev) == n and all(type(v) is sb.ExtensionFieldElement for v in ev)
    planes = limb_planes(ev)
    for l in range(3):
        sc.check_evaluate(dom, coeffs[l], planes[l])


@pytest.mark.parametrize("n", [257, 4100])
def test_equal_points_in_different_subtrees(sb, lib, n):
    """position n - 1 repeats position 0 and position 128 repeats position 127: interpolation is undefined (the C entry reports
    the zero of the batch inverse and writes nothing, the wrapper raises), the zerofier and evaluation are what they were.  No free
    points here: a repeated 0 would give the last, partial subtree a constant term of 0, which hides what is done to it"""
    dom = sc.with_equal(sc.ragged(n, SEED + 1), [(0, n - 1), (127, 128)])
    batch, in_stride, out_stride = 3, n + 5, n + 3
    values = sc.columns(batch, n, SEED + 4)
    with AbiTree(lib, dom) as tree:
        src, host = strided_input(values, in_stride)
        out = Arena(batch=batch, stride=out_stride, n=n)
        assert lib.bfs_ptree_interpolate(tree.handle, src.ptr, in_stride, batch, out.ptr, out_stride, 0) == BFS_ERR_ZERO_IN_BATCH_INVERSE
        after = out.contained([("values", host, src.to_numpy()), ("points", tree.host, tree.points.to_numpy())])
        assert (after == np.uint64(PAINT_WORD)).all()
    tree = tree_of(sb, dom)
    with pytest.raises(AssertionError):
        tree.interpolate(sb.BaseArray.from_numpy(values[0]))
    z = tree.zerofier().to_numpy()
    sc.check_zerofier(dom, z)
    sc.check_double_roots(dom, z, (0, 127))
    for m in (n, n + 129):
        coeffs = sc.column("random", m, SEED + m)
        sc.check_evaluate(dom, coeffs, tree.evaluate(sb.BaseArray.from_numpy(coeffs)).to_numpy())


def test_one_tree_serves_many_calls(sb):
    """evaluate, interpolate, evaluate again on one handle with other batch sizes in between: the kept transforms are read only"""
    n = 1000
    dom = ragged_domain(n)
    tree = tree_of(sb, dom)
    coeffs = sc.column("random", n + 129, SEED + 5)
    values = sc.columns(3, n, SEED + 6)
    seven = sc.columns(7, n - 1, SEED + 7)
    first = tree.evaluate(sb.BaseArray.from_numpy(coeffs)).to_numpy()
    three = tree.interpolate(sb.BaseArray.from_numpy(values)).to_numpy()
    wide = tree.evaluate(sb.BaseArray.from_numpy(seven)).to_numpy()
    one = tree.interpolate(sb.BaseArray.from_numpy(values[0])).to_numpy()
    again = tree.evaluate(sb.BaseArray.from_numpy(coeffs)).to_numpy()
    zero = tree.zerofier().to_numpy()
    sc.check_evaluate(dom, coeffs, first)
    assert (again == first).all() and (one == three[0]).all()
    for b in range(3):
        sc.check_interpolant(dom, values[b], three[b])
    for b in range(7):
        sc.check_evaluate(dom, seven[b], wide[b])
    sc.check_zerofier(dom, zero)
