"""The checker of tests/painted.py on numpy snapshots, without a GPU: a change planted in every region outside the results is
reported with that region's name and the offset inside it, a clean snapshot passes, a result that holds the paint value is no
violation, and a changed input is reported by its name."""
import numpy as np
import pytest

import painted
from painted import GUARD_WORDS, PAINT_BYTE, PAINT_WORD, Layout, Violation


def _after(layout, seed=1):
    """a snapshot after a well-behaved call: residues in every result range, paint everywhere else"""
    rng = np.random.default_rng(seed)
    snap = layout.painted()
    for k in range(len(layout.results)):
        r = layout.result(snap, k)
        r[:] = rng.integers(0, painted.P if layout.dtype == np.uint64 else 256, r.size, dtype=np.uint64).astype(layout.dtype)
    return snap


def test_the_paint_is_no_residue_and_the_guards_cover_a_workgroup():
    assert PAINT_WORD >= painted.P and PAINT_WORD < 1 << 64
    assert GUARD_WORDS == 4096
    words, octets = Layout(batch=3, stride=10, n=7), Layout(batch=1, stride=64, n=64, dtype=np.uint8)
    assert words.guard == 4096 and octets.guard == 4096 * 8
    assert (words.painted() == np.uint64(PAINT_WORD)).all() and (octets.painted() == PAINT_BYTE).all()
    assert words.total == 2 * 4096 + 30 and octets.total % 8 == 0


def test_regions_of_the_default_layout():
    lay = Layout(batch=3, stride=12, n=7)
    g = lay.guard
    assert lay.regions == [("front guard", 0, g), ("gap 0", g + 7, g + 12), ("gap 1", g + 19, g + 24), ("gap 2", g + 31, g + 36),
                           ("back guard", g + 36, 2 * g + 36)]
    assert Layout(batch=2, stride=5, n=5).regions == [("front guard", 0, 4096), ("back guard", 4096 + 10, 8192 + 10)]
    # explicit result ranges: a Merkle node array of 8 slots with digest 0 and two absent leaves left alone
    tree = Layout(dtype=np.uint8, results=[(64, 5 * 64)], payload=8 * 64)
    g = tree.guard
    assert tree.regions == [("front guard", 0, g), ("head gap", g, g + 64), ("gap 0", g + 6 * 64, g + 8 * 64), ("back guard", g + 8 * 64, 2 * g + 8 * 64)]


@pytest.mark.parametrize("dtype", [np.uint64, np.uint8])
def test_a_clean_snapshot_passes(dtype):
    lay = Layout(batch=3, stride=24, n=17, dtype=dtype)
    before, after = lay.painted(), _after(lay)
    assert lay.violation(before, after) is None
    lay.check(before, after, inputs=[("a", np.arange(5), np.arange(5))])
    assert (lay.rows(after) != lay.paint).any()
    assert lay.rows(after).shape == (3, 17)


@pytest.mark.parametrize("dtype", [np.uint64, np.uint8])
def test_a_planted_change_in_each_region_is_named_with_its_offset(dtype):
    lay = Layout(batch=3, stride=24, n=17, dtype=dtype)
    before, clean = lay.painted(), _after(lay)
    seen = []
    for name, start, stop in lay.regions:
        for offset in sorted({0, (stop - start) // 2, stop - start - 1}):
            after = clean.copy()
            after[start + offset] ^= 1
            v = lay.violation(before, after)
            assert isinstance(v, Violation) and (v.region, v.offset, v.index) == (name, offset, start + offset), (name, offset, v)
            assert v.before == lay.paint and v.after == lay.paint ^ 1
            with pytest.raises(Violation, match=name):
                lay.check(before, after)
        seen.append(name)
    assert seen == ["front guard", "gap 0", "gap 1", "gap 2", "back guard"]


def test_the_first_change_in_address_order_is_the_one_reported():
    lay = Layout(batch=2, stride=9, n=4)
    before, after = lay.painted(), _after(lay)
    g = lay.guard
    after[g + 9 + 6] = 0                 # gap 1, offset 2
    after[g + 5] = 0                     # gap 0, offset 1
    after[2 * g + 18 - 1] = 0            # back guard, its last word
    v = lay.violation(before, after)
    assert (v.region, v.offset) == ("gap 0", 1)


@pytest.mark.parametrize("dtype", [np.uint64, np.uint8])
def test_a_result_that_holds_the_paint_value_is_no_violation(dtype):
    lay = Layout(batch=2, stride=11, n=8, dtype=dtype)
    before, after = lay.painted(), _after(lay)
    lay.result(after, 0)[3] = lay.paint
    lay.result(after, 1)[:] = lay.paint          # a whole result left as it was: containment does not judge values
    assert lay.violation(before, after) is None
    lay.check(before, after)


def test_a_write_that_stores_the_old_value_cannot_be_seen_and_a_changed_prefilled_gap_can():
    """the checker compares snapshots, so an arena whose gaps were filled with data (an accumulator) is checked the same way"""
    lay = Layout(batch=1, stride=40, n=10)
    before = lay.painted()
    before[lay.guard + 10:lay.guard + 40] = np.arange(30, dtype=np.uint64)
    after = before.copy()
    lay.result(after)[:] = 5
    assert lay.violation(before, after) is None
    after[lay.guard + 25] += np.uint64(1)
    v = lay.violation(before, after)
    assert (v.region, v.offset, v.before, v.after) == ("gap 0", 15, 15, 16)


def test_a_changed_input_is_reported_by_name():
    lay = Layout(batch=1, stride=8, n=8)
    before, after = lay.painted(), _after(lay)
    a = np.arange(100, dtype=np.uint64)
    b = a.copy()
    b[41] = 7
    b[90] = 7
    with pytest.raises(Violation) as e:
        lay.check(before, after, inputs=[("points", a, a.copy()), ("values", a, b)])
    assert (e.value.region, e.value.offset, e.value.before, e.value.after) == ("input values", 41, 41, 7)
    # a stray write is reported before a changed input
    after[0] = 0
    with pytest.raises(Violation, match="front guard"):
        lay.check(before, after, inputs=[("values", a, b)])


def test_snapshots_of_another_shape_are_refused():
    lay = Layout(batch=1, stride=8, n=8)
    with pytest.raises(AssertionError):
        lay.violation(lay.painted(), lay.painted()[:-1])
    with pytest.raises(AssertionError):
        Layout(results=[(4, 4), (6, 2)], payload=10)
