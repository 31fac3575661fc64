"""Opening each committed polynomial at its own set of points (stark_brainfuck_amd/pcs.py: open_at / verify_at; include/bfstark_open.h),
host side, no GPU: the kernels' per-thread code (csrc/deep_core.hpp through tests/emu/emu_deep_groups.cpp) against the CPython model
(tests/pcs_groups_model.py), the host verifier against the model's proofs, its refusals, the plan's validation.  Arithmetic is exact:
every comparison is for equality."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

from conftest import ROOT

import pcs_groups_cases as cases
import pcs_groups_model as gmodel
import pcs_model as model

P = model.P
PROTOCOL = [(N, mode) for N in (64, 256) for mode in sorted(cases.MODES)]
IDS = ["%d-%s" % c for c in PROTOCOL]
PAINT = 0xA5A5A5A5


@pytest.fixture(scope="session")
def sb():
    from stark_brainfuck_amd import build
    build.build_library()
    import stark_brainfuck_amd
    return stark_brainfuck_amd


@pytest.fixture(scope="module")
def emu():
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    from build_emu import build_emulation
    e = ctypes.CDLL(build_emulation())
    u64, vp, u = ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint
    e.emu_deep_eval_columns.argtypes = [vp, vp, u, vp, u, vp]
    e.emu_deep_quotient_groups.argtypes = [vp, vp, u, u64, u, u64, u64, vp, vp, u, vp, u, vp, vp, vp, vp, u64]
    e.emu_deep_groups_share.argtypes = [u]
    e.emu_deep_groups_share.restype = u
    return e


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _flat(triples):
    return np.array([v for z in triples for v in z], dtype=np.uint64)


# ------------------------------------------------------------------------------------------------ 1. the emulated quotient
def emulated_quotient(emu, case, out_stride=None):
    N = case["N"]
    out_stride = N if out_stride is None else out_stride
    args = cases.kernel_arguments(case)
    columns = [np.ascontiguousarray(c) for c in args["columns"]]
    m = len(columns)
    pointers = (ctypes.c_void_p * m)(*[c.ctypes.data for c in columns])
    is_ext = (ctypes.c_int * m)(*[int(c.ndim == 2) for c in columns])
    u32 = lambda values: np.array(values, dtype=np.uint32)
    out = np.full((3, out_stride), PAINT, dtype=np.uint64)
    rc = emu.emu_deep_quotient_groups(pointers, is_ext, m, case["stride"], N.bit_length() - 1, cases.OFFSET, case["omega"], _ptr(u32(args["group_columns"])),
                                      _ptr(u32(args["group_pairs"])), len(args["group_columns"]), _ptr(_flat(args["points"])), len(args["points"]),
                                      _ptr(u32(args["pair_point"])), _ptr(_flat(args["pair_values"])), _ptr(np.array(case["lam"], dtype=np.uint64)),
                                      _ptr(out), out_stride)
    assert rc == 0
    return out


def test_the_case_files_share_is_the_kernels(emu):
    assert {n: emu.emu_deep_groups_share(n) for n in range(1, 9)} == cases.SHARE
    assert 2 * cases.SHARE[1] in cases.QUOTIENT_SIZES and 2 * cases.SHARE[8] in cases.QUOTIENT_SIZES and 2 * cases.SHARE[8] in cases.MAX_SIZES


@pytest.mark.parametrize("N", cases.QUOTIENT_SIZES)
@pytest.mark.parametrize("layout", sorted(cases.LAYOUTS))
@pytest.mark.parametrize("k", cases.POINT_COUNTS)
def test_one_group_of_all_columns_is_the_old_formula(emu, N, layout, k):
    case = cases.plan_one(N, layout, k)
    plan = case["plan"]
    assert plan.base == [[j * plan.m for j in range(k)]]
    assert np.array_equal(case["g"], model.quotient(case["columns"], N, cases.OFFSET, case["omega"], plan.points, case["Y"][0], case["lam"]))
    if N <= 256:      # the groups model itself, where it is cheap
        assert np.array_equal(gmodel.quotient(case["columns"], N, cases.OFFSET, case["omega"], plan, case["Y"], case["lam"]), case["g"])
    assert np.array_equal(emulated_quotient(emu, case), case["g"])


@pytest.mark.parametrize("N", cases.QUOTIENT_SIZES)
def test_emulated_tables_plan_is_the_models(emu, N):
    case = cases.plan_tables(N)
    assert np.array_equal(emulated_quotient(emu, case), case["g"])


@pytest.mark.parametrize("N", cases.MAX_SIZES)
def test_emulated_plan_at_every_limit_is_the_models(emu, N):
    case = cases.plan_max(N)
    assert np.array_equal(emulated_quotient(emu, case), case["g"])


@pytest.mark.parametrize("N", cases.QUOTIENT_SIZES)
def test_emulated_singletons_are_one_group_at_one_point(emu, N):
    case = cases.plan_singletons(N)
    assert case["plan"].base == [[g] for g in range(5)]
    assert case["g"] is cases.plan_one(N, "mixed", 1)["g"]
    assert np.array_equal(emulated_quotient(emu, case), case["g"])


def test_emulated_quotient_with_strides(emu):
    case = cases.plan_tables(256, stride=256 + 24)
    out = emulated_quotient(emu, case, out_stride=256 + 40)
    assert np.array_equal(out[:, :256], case["g"]) and np.all(out[:, 256:] == PAINT)


# ------------------------------------------------------------------------------------------------ 2. the emulated evaluation
@pytest.mark.parametrize("name", sorted(cases.EVAL_CASES))
@pytest.mark.parametrize("k", cases.EVAL_POINT_COUNTS)
def test_emulated_evaluation_of_separate_columns_is_the_models(emu, name, k):
    columns, points, reference = cases.eval_case(name)
    columns = [np.ascontiguousarray(c) for c in columns]
    count = len(columns)
    pointers = (ctypes.c_void_p * count)(*[c.ctypes.data for c in columns])
    lengths = np.array([c.size for c in columns], dtype=np.uint64)
    out = np.full(3 * count * k, PAINT, dtype=np.uint64)
    assert emu.emu_deep_eval_columns(pointers, _ptr(lengths), count, _ptr(_flat(points[:k])), k, _ptr(out)) == 0
    got = [[tuple(int(v) for v in out[(b * k + j) * 3:(b * k + j) * 3 + 3]) for j in range(k)] for b in range(count)]
    assert got == [row[:k] for row in reference]


# ------------------------------------------------------------------------------------------------ 3. the protocol
def _fri(sb, N, mode):
    a, coset, bits = cases.MODES[mode]
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    assert BF.generator().value == cases.OFFSET
    return sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, cases.EXPANSION, cases.T, XF, folding_factor=a, coset_leaves=coset, grinding_bits=bits)


def _elements(pc, values):
    return [[[pc.xfield.from_limbs(list(v)) for v in per_point] for per_point in per_group] for per_group in values]


def _package_verdict(sb, N, mode, data, root, plan, values, edit=None):
    """PolynomialCommitment.verify_at on a serialised stream; edit(objects) -> objects tampers with the deserialised list"""
    pc = sb.PolynomialCommitment(_fri(sb, N, mode))
    ps = sb.ProofStream().deserialize(data)
    if edit is not None:
        ps.objects = edit(list(ps.objects))
    assert ps.pull() is not None                    # the commitment's root: the caller's to read
    return pc.verify_at(root, plan, _elements(pc, values), ps)


def _model_verdict(sb, o, proof, root=None, plan=None, values=None):
    import test_pcs_host as host
    a, coset, _ = cases.MODES[proof["mode"]]
    return gmodel.verify(o, proof["proof_stream"].objects, proof["root"] if root is None else root, proof["raw_plan"] if plan is None else plan,
                         proof["values"] if values is None else values, proof["N"], cases.OFFSET, proof["omega"], cases.T, a, coset,
                         host._fri_verify(sb, proof["N"], proof["mode"]))


@pytest.mark.parametrize("N,mode", PROTOCOL, ids=IDS)
def test_both_verifiers_accept_the_models_proof(sb, oracle, N, mode):
    proof = cases.model_proof(N, mode)
    assert len(proof["plan"].points) == 2 and proof["plan"].shape == [((0, 2, 4), (0, 1)), ((1,), (1, 0)), ((3,), (0,))]
    assert _model_verdict(sb, oracle, proof) == (True, "accepted")
    assert _package_verdict(sb, N, mode, proof["bytes"], proof["root"], proof["raw_plan"], proof["values"]) is True


def _bump(element):
    limbs = element.limbs()
    return element.field.from_limbs([(limbs[0] + 1) % P, limbs[1], limbs[2] or 1])


def _edit_value(objects):
    values = [[list(per_point) for per_point in per_group] for per_group in objects[3]]
    values[1][1][0] = _bump(values[1][1][0])
    return objects[:3] + [values] + objects[4:]


def _edit_row(objects):
    assert isinstance(objects[5], tuple) and isinstance(objects[6], list)
    row = list(objects[5])
    row[0] = _bump(row[0])
    return objects[:5] + [tuple(row)] + objects[6:]


def _edit_quotient_opening(coset):
    def edit(objects):
        leaf = objects[7]
        if coset:
            assert isinstance(leaf, tuple)
            leaf = tuple(_bump(e) for e in leaf)
        else:
            leaf = _bump(leaf)
        return objects[:7] + [leaf] + objects[8:]
    return edit


def _edit_shape(objects):
    shape = list(objects[2])
    assert shape[0] == ((0, 2, 4), (0, 1)) and shape[2] == ((3,), (0,))
    shape[0], shape[2] = ((0, 2), (0, 1)), ((3, 4), (0,))
    return objects[:2] + [shape] + objects[3:]


def other_plans(plan):
    """the caller's plan changed three ways"""
    (c0, p0), (c1, p1), (c2, p2) = plan
    moved = [(c0[:-1], p0), (c1, p1), (sorted(c2 + c0[-1:]), p2)]
    swapped = [(c0, p1), (c1, p0), (c2, p2)]
    z = p0[0]
    changed = [(c0, [model.xadd(z, (1, 0, 0)), p0[1]]), (c1, p1), (c2, p2)]
    return {"moved": moved, "swapped": swapped, "changed": changed}


@pytest.mark.parametrize("N,mode", [(64, "default"), (256, "coset8")], ids=["64-default", "256-coset8"])
def test_the_verifier_refuses_tampered_streams_and_other_statements(sb, oracle, N, mode, capsys):
    proof = cases.model_proof(N, mode)
    data, root, plan, values = proof["bytes"], proof["root"], proof["raw_plan"], proof["values"]
    verdicts = {"untouched": _package_verdict(sb, N, mode, data, root, plan, values)}
    capsys.readouterr()
    refusals = {"value": dict(edit=_edit_value), "row": dict(edit=_edit_row), "opening": dict(edit=_edit_quotient_opening(cases.MODES[mode][1])),
                "shape": dict(edit=_edit_shape), "root": dict(root=bytes(64))}
    for name, other in other_plans(plan).items():
        refusals[name] = dict(plan=other)
    for name, change in refusals.items():
        verdicts[name] = _package_verdict(sb, N, mode, data, change.get("root", root), change.get("plan", plan), values, edit=change.get("edit"))
        printed = capsys.readouterr().out
        assert printed.count("\n") == 1, (name, printed)          # one line per refusal
    assert verdicts == dict({name: False for name in refusals}, untouched=True)
    assert _model_verdict(sb, oracle, proof, root=bytes(64)) == (False, "root")
    others = other_plans(plan)
    assert _model_verdict(sb, oracle, proof, plan=others["moved"]) == (False, "shape")
    assert _model_verdict(sb, oracle, proof, plan=others["swapped"]) == (False, "points")          # (the order of first appearance changes)
    assert _model_verdict(sb, oracle, proof, plan=others["changed"]) == (False, "points")


@pytest.mark.parametrize("N,mode", sorted(cases.FORCED_SEEDS), ids=["%d-%s" % c for c in sorted(cases.FORCED_SEEDS)])
def test_a_forced_proof_is_refused_by_both_verifiers(sb, oracle, N, mode, capsys):
    seed = cases.FORCED_SEEDS[N, mode]
    honest, forced = cases.model_proof(N, mode, seed=seed), cases.model_proof(N, mode, forced=True, seed=seed)
    differing = [(g, j, r) for g, per_group in enumerate(forced["values"]) for j, per_point in enumerate(per_group) for r, v in enumerate(per_point)
                 if v != honest["values"][g][j][r]]
    assert differing == [(1, 1, 0)]                   # one false value, in one group, at that group's second point
    assert forced["root"] == honest["root"]
    assert _model_verdict(sb, oracle, forced)[0] is False
    capsys.readouterr()
    assert _package_verdict(sb, N, mode, forced["bytes"], forced["root"], forced["raw_plan"], forced["values"]) is False
    assert capsys.readouterr().out.count("\n") == 1


# ------------------------------------------------------------------------------------------------ 4. the plan's validation
def test_bad_plans_are_refused_before_any_library_call(sb):
    N = 64
    pc = sb.PolynomialCommitment(_fri(sb, N, "default"))
    committed = types.SimpleNamespace(polys=[None] * 5)          # (no commitment in HBM, no library call: refused first)
    z = [(1 + i, 2, 3) for i in range(9)]
    omega = pc.xfield.modulus.coefficients[0].field.primitive_nth_root(N).value
    inside = (cases.OFFSET * pow(omega, 5, P) % P, 0, 0)
    bad = {"overlapping groups": [([0, 1, 2], [z[0]]), ([2, 3, 4], [z[1]])],
           "a missing column": [([0, 1], [z[0]]), ([3, 4], [z[1]])],
           "a column too many": [([0, 1, 2], [z[0]]), ([3, 4, 5], [z[1]])],
           "descending columns": [([1, 0, 2, 3, 4], [z[0]])],
           "an empty group": [([0, 1, 2, 3, 4], [z[0]]), ([], [z[1]])],
           "no point": [([0, 1, 2, 3, 4], [])],
           "five points in a group": [([0, 1, 2, 3, 4], z[:5])],
           "a domain point": [([0, 1, 2], [z[0]]), ([3, 4], [z[1], inside])],
           "a point twice in one group": [([0, 1, 2], [z[0]]), ([3, 4], [z[1], (1 + 1 + P, 2, 3)])]}
    wide = types.SimpleNamespace(polys=[None] * 9)
    bad_wide = {"9 groups": [([c], [z[0]]) for c in range(9)],
                "17 pairs": [([c], z[:4]) for c in range(4)] + [([4, 5, 6, 7, 8], [z[0]])],
                "9 points": [([c], [z[2 * c], z[2 * c + 1]]) for c in range(4)] + [([4, 5, 6, 7, 8], [z[8]])]}
    for who, plans in ((committed, bad), (wide, bad_wide)):
        for name, plan in plans.items():
            ps = sb.ProofStream()
            with pytest.raises(ValueError):
                pc.open_at(who, plan, ps)
            assert ps.objects == [], name
    good = pc.plan([([0, 1, 2], [z[0], z[1]]), ([3, 4], [z[1]])], 5)
    assert good.points == [z[0], z[1]] and good.shape == [((0, 1, 2), (0, 1)), ((3, 4), (1,))] and good.base == [[0, 3], [6]]
    limit = pc.plan([([c], z[:2]) for c in range(8)], 8)          # 8 groups, 16 pairs
    assert limit.pairs == 16 and len(pc.plan([([c], [z[c]]) for c in range(8)], 8).points) == 8


def test_a_bad_plan_is_one_refusal_line_of_the_verifier(sb, capsys):
    pc = sb.PolynomialCommitment(_fri(sb, 64, "default"))
    assert pc.verify_at(bytes(64), [([0, 2], [(1, 2, 3)])], [[[(0, 0, 0)] * 2]], sb.ProofStream()) is False
    assert capsys.readouterr().out.count("\n") == 1


def test_column_of_is_the_inverse_of_order(sb):
    from stark_brainfuck_amd.pcs import Commitment
    is_ext = [False, False, True, False, True]
    order = [2, 4, 0, 1, 3]
    committed = Commitment([None] * 5, is_ext, order, None, 64, None)
    assert [committed.column_of(position) for position in range(5)] == [2, 3, 0, 4, 1]
    assert [order[committed.column_of(position)] for position in range(5)] == list(range(5))


def test_the_plan_goes_through_the_transcript_as_the_model_pushes_it(sb, oracle):
    """lists of tuples of plain ints: the same bytes from the package's stream and from the model's"""
    shape = [((0, 2, 4), (0, 1)), ((1,), (1, 0)), ((3,), (0,))]
    ps, ref = sb.ProofStream(), oracle.ProofStreamOracle()
    ps.push(shape)
    ref.push(shape)
    assert ps.serialize() == ref.serialize()
    assert sb.ProofStream().deserialize(ps.serialize()).pull() == shape
