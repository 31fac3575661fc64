"""When a list call of fast_zerofier / fast_evaluate / fast_interpolate goes to the GPU subproduct tree (pure host logic: no GPU)."""
import importlib

from stark_brainfuck_amd import BaseField, ExtensionField

ntt_mod = importlib.import_module("stark_brainfuck_amd.ntt")       # (the package attribute `ntt` is the function)
XF = ExtensionField.main()
F = XF._base()


def test_size_rule():
    w = F.primitive_nth_root(128)
    small = [F(i) for i in range(ntt_mod.TREE_MIN_POINTS - 1)]
    assert ntt_mod._tree_points(small, w, 128) is None
    at_min = [F(i) for i in range(ntt_mod.TREE_MIN_POINTS)]
    assert ntt_mod._tree_points(at_min, w, 128) == list(range(ntt_mod.TREE_MIN_POINTS))
    assert ntt_mod._tree_points([F(i) for i in range(127)], w, 128) == list(range(127))
    # len(domain) == root_order: the recursion's largest product would wrap in fast_multiply's transform
    assert ntt_mod._tree_points([F(i) for i in range(128)], w, 128) is None


def test_type_rule():
    n = 100
    w = F.primitive_nth_root(128)
    base = [F(i + 1) for i in range(n)]
    lifted = [XF.lift(x) for x in base]
    xvals = [XF.from_limbs([i, 1, 2]) for i in range(n)]
    assert ntt_mod._tree_points(base, w, 128, base) == list(range(1, n + 1))
    assert ntt_mod._tree_points(lifted, XF.lift(w), 128, xvals) == list(range(1, n + 1))
    assert ntt_mod._tree_points(lifted, XF.lift(w), 128, lifted) == list(range(1, n + 1))
    # mixed element types stay on the recursion (which raises for them)
    assert ntt_mod._tree_points(base, XF.lift(w), 128) is None
    assert ntt_mod._tree_points(lifted, w, 128) is None
    assert ntt_mod._tree_points(base, w, 128, xvals) is None
    assert ntt_mod._tree_points(lifted, XF.lift(w), 128, base) is None
    assert ntt_mod._tree_points(base[:-1] + [lifted[-1]], w, 128) is None
    # a genuine extension point: out of the tree's scope
    assert ntt_mod._tree_points(lifted[:-1] + [XF.from_limbs([1, 2, 3])], XF.lift(w), 128) is None


def test_subproduct_tree_is_exported():
    import stark_brainfuck_amd as sb
    assert sb.SubproductTree is ntt_mod.SubproductTree and "SubproductTree" in sb.__all__
