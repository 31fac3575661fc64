"""Openings across commitments (stark_brainfuck_amd/pcs.py: open_rounds / verify_rounds; include/bfstark_rounds.h), host side, no GPU:
the library's split rule and its launches' per-thread code (csrc/deep_core.hpp through tests/emu/emu_deep_rounds.cpp) against the CPython
model (tests/pcs_rounds_model.py), the host verifier against the model's proofs, its refusals, the plan's validation.  Arithmetic is
exact: every comparison is for equality."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

from conftest import ROOT

import pcs_groups_model as gmodel
import pcs_model as model
import pcs_rounds_cases as cases
import pcs_rounds_model as rmodel

P = model.P
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
    e.emu_deep_quotient_rounds.argtypes = [vp, vp, u, u64, u, u64, u64, vp, vp, u, vp, u, vp, vp, vp, vp, u64]
    e.emu_deep_rounds_split.argtypes = [u, vp, vp, u, u, vp, vp]
    e.emu_deep_rounds_limits.argtypes = [vp]
    return e


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _flat(triples):
    return np.array([v for z in triples for v in z], dtype=np.uint64)


def _u32(values):
    return np.array(values, dtype=np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the split rule
def emulated_split(emu, plan):
    """deep_rounds_split on a plan -> per launch dict(groups, columns, pairs, points), or None when the plan is refused"""
    group_columns, group_pairs = [len(c) for c, _ in plan.groups], [len(i) for _, i in plan.groups]
    out = np.full(16 * len(plan.groups), 0xDEAD, dtype=np.uint32)
    count = emu.emu_deep_rounds_split(plan.m, _ptr(_u32(group_columns)), _ptr(_u32(group_pairs)), len(plan.groups), len(plan.points),
                                      _ptr(_u32([p for _, i in plan.groups for p in i])), _ptr(out))
    if count < 0:
        return None
    launches = []
    for l in range(count):
        first_group, n_groups, first_column, n_columns, first_pair, n_pairs, n_points = (int(v) for v in out[16 * l:16 * l + 7])
        launches.append({"groups": list(range(first_group, first_group + n_groups)), "first_column": first_column, "columns": n_columns,
                         "first_pair": first_pair, "pairs": n_pairs, "points": [int(v) for v in out[16 * l + 8:16 * l + 8 + n_points]]})
    return launches


def test_the_models_limits_are_the_librarys(emu, sb):
    from stark_brainfuck_amd import pcs
    out = np.zeros(8, dtype=np.uint32)
    assert emu.emu_deep_rounds_limits(_ptr(out)) == 8
    assert [int(v) for v in out] == [96, 24, 24, 48, rmodel.LAUNCH_COLUMNS, rmodel.LAUNCH_GROUPS, rmodel.LAUNCH_POINTS, rmodel.LAUNCH_PAIRS]
    assert pcs.ROUNDS_LIMITS == (24, 24, 48, 96, 32) and pcs.PLAN_LIMITS == (8, 8, 16, 32, 32) and pcs.MAX_COMMITMENTS == 4


@pytest.mark.parametrize("name", sorted(cases.CASE_SIZES))
def test_the_split_is_the_rules_in_plan_order_within_every_limit(emu, name):
    case = cases.case(name, 64)
    plan = case["plan"]
    launches = emulated_split(emu, plan)
    assert [l["groups"] for l in launches] == case["launches"] == rmodel.launches(plan)
    assert [g for l in launches for g in l["groups"]] == list(range(len(plan.groups)))          # plan order, every group once
    column = pair = 0
    for l in launches:
        groups = [plan.groups[g] for g in l["groups"]]
        assert (l["first_column"], l["first_pair"]) == (column, pair)
        assert l["columns"] == sum(len(c) for c, _ in groups) <= 32 and 1 <= len(groups) <= 8
        assert l["pairs"] == sum(len(i) for _, i in groups) <= 16
        assert l["points"] == list(dict.fromkeys(p for _, i in groups for p in i)) and len(l["points"]) <= 8      # re-indexed by first appearance
        column, pair = column + l["columns"], pair + l["pairs"]
    assert column == plan.m
    if name != "fits" and name != "rounds3":
        assert len(launches) > 1                          # the case really accumulates
    # the clause that closes the first launch: the next group would break exactly the limit the case is named after
    if len(launches) > 1:
        first, (next_columns, next_points) = launches[0], plan.groups[launches[1]["groups"][0]]
        broken = {"by_columns": first["columns"] + len(next_columns) > 32, "by_groups": len(first["groups"]) + 1 > 8,
                  "by_pairs": first["pairs"] + len(next_points) > 16, "by_points": len(set(first["points"]) | set(next_points)) > 8,
                  "max": len(set(first["points"]) | set(next_points)) > 8}
        # (by_points' ninth group is also a ninth group; `max` closes on the points alone, after seven groups)
        assert broken[name] and sum(broken[k] for k in ("by_columns", "by_groups", "by_pairs", "by_points")) == (2 if name == "by_points" else 1)


@pytest.mark.parametrize("name", ["plan_max", "plan_tables"])
def test_a_plan_within_the_one_launch_limits_is_one_launch_with_its_points_in_order(emu, name):
    """bfsx_deep_quotient_groups goes through the same split: every bound of the split is one of its limits, so its plans -- the one at
    every limit at once among them -- are one launch of all groups, columns and pairs, the points 0 .. n_points - 1 as the plan has them"""
    import pcs_groups_cases as gcases
    plan = getattr(gcases, name)(64)["plan"]
    if name == "plan_max":
        assert (plan.m, len(plan.groups), len(plan.points), sum(len(i) for _, i in plan.groups)) == (32, 8, 8, 16)
    launches = emulated_split(emu, plan)
    assert len(launches) == 1
    assert launches[0] == {"groups": list(range(len(plan.groups))), "first_column": 0, "columns": plan.m, "first_pair": 0,
                           "pairs": sum(len(i) for _, i in plan.groups), "points": list(range(len(plan.points)))}


def test_the_split_refuses_what_the_entry_refuses(emu):
    z = [(1 + i, 2, 3) for i in range(25)]
    assert emulated_split(emu, gmodel.Plan([([c], [z[0]]) for c in range(24)])) is not None
    assert emulated_split(emu, gmodel.Plan([([c], [z[0]]) for c in range(25)])) is None                    # 25 groups
    assert emulated_split(emu, gmodel.Plan([(list(range(33)), [z[0]])])) is None                            # a group of 33 columns
    assert emulated_split(emu, gmodel.Plan([([c], z[:4]) for c in range(12)] + [([12], [z[0]])])) is None      # 49 pairs
    assert emulated_split(emu, gmodel.Plan([(list(range(32 * r, 32 * r + 32)), [z[0]]) for r in range(3)] + [([96], [z[1]])])) is None      # 97 columns


# ------------------------------------------------------------------------------------------------ 2. the emulated quotient
def emulated_quotient(emu, case, out_stride=None, paint=PAINT):
    N = case["N"]
    out_stride = N if out_stride is None else out_stride
    args = cases.kernel_arguments(case)
    columns = [np.ascontiguousarray(c) for c in args["columns"]]
    m = len(columns)
    pointers = (ctypes.c_void_p * m)(*[c.ctypes.data for c in columns])
    is_ext = (ctypes.c_int * m)(*[int(c.ndim == 2) for c in columns])
    out = np.full((3, out_stride), paint, dtype=np.uint64)
    count = emu.emu_deep_quotient_rounds(pointers, is_ext, m, case["stride"], N.bit_length() - 1, cases.OFFSET, case["omega"], _ptr(_u32(args["group_columns"])),
                                         _ptr(_u32(args["group_pairs"])), len(args["group_columns"]), _ptr(_flat(args["points"])), len(args["points"]),
                                         _ptr(_u32(args["pair_point"])), _ptr(_flat(args["pair_values"])), _ptr(np.array(case["lam"], dtype=np.uint64)),
                                         _ptr(out), out_stride)
    return out, count


@pytest.mark.parametrize("name,N", cases.ALL, ids=cases.IDS)
def test_emulated_launches_add_up_to_the_models_quotient(emu, name, N):
    case = cases.case(name, N)
    out, count = emulated_quotient(emu, case)
    assert count == len(case["launches"])
    assert np.array_equal(out, case["g"])


def test_the_fitting_plan_is_the_groups_kernels_case(emu):
    import pcs_groups_cases as gcases
    assert cases.case("fits", 64)["g"] is gcases.plan_tables(64)["g"]


@pytest.mark.parametrize("name", ["by_points", "max"])
def test_emulated_quotient_with_strides_leaves_the_words_in_between_alone(emu, name):
    N = 64
    case = cases.case(name, N, stride=N + 24)
    out, count = emulated_quotient(emu, case, out_stride=N + 40)
    assert count == len(case["launches"]) > 1
    assert np.array_equal(out[:, :N], case["g"]) and np.all(out[:, N:] == PAINT)


@pytest.mark.parametrize("name", ["by_columns", "by_points"])
def test_the_first_launch_does_not_read_the_output(emu, name):
    case = cases.case(name, 512)
    assert np.array_equal(emulated_quotient(emu, case, paint=0)[0], emulated_quotient(emu, case, paint=P - 1)[0])


# ------------------------------------------------------------------------------------------------ 3. the protocol
def _fri(sb, N, mode):
    a, coset, bits = cases.MODES[mode]
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    assert BF.generator().value == cases.OFFSET
    return sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, cases.EXPANSION, cases.T, XF, folding_factor=a, coset_leaves=coset, grinding_bits=bits)


def _elements(pc, values):
    return [[[pc.xfield.from_limbs(list(v)) for v in per_point] for per_point in per_group] for per_group in values]


def _package_verdict(sb, N, mode, data, roots, widths, plan, values, edit=None):
    """PolynomialCommitment.verify_rounds on a serialised stream; edit(objects) -> objects tampers with the deserialised list"""
    pc = sb.PolynomialCommitment(_fri(sb, N, mode))
    ps = sb.ProofStream().deserialize(data)
    if edit is not None:
        ps.objects = edit(list(ps.objects))
    for at in range(cases.START):                    # the roots and what lies between them: the caller's to read
        assert ps.pull() is not None
    return pc.verify_rounds(roots, widths, plan, _elements(pc, values), ps)


def _model_verdict(sb, o, proof, roots=None, widths=None, plan=None, values=None):
    import test_pcs_host as host
    a, coset, _ = cases.MODES[proof["mode"]]
    return rmodel.verify(o, proof["proof_stream"].objects, proof["start"], proof["roots"] if roots is None else roots,
                         proof["widths"] if widths is None else widths, proof["raw_plan"] if plan is None else plan,
                         proof["values"] if values is None else values, proof["N"], cases.OFFSET, proof["omega"], cases.T, a, coset,
                         host._fri_verify(sb, proof["N"], proof["mode"]))


@pytest.mark.parametrize("N,mode", cases.PROTOCOL, ids=cases.PROTOCOL_IDS)
def test_both_verifiers_accept_the_models_proof(sb, oracle, N, mode):
    proof = cases.model_proof(N, mode)
    assert proof["widths"] == [16, 9, 7] and len(proof["plan"].points) == 4 and len(proof["roots"]) == 3
    firsts = rmodel.first_columns(proof["widths"])
    assert any(len({sum(c >= f for f in firsts) for c in columns}) > 1 for columns, _ in proof["plan"].groups)      # a group mixes commitments
    assert _model_verdict(sb, oracle, proof) == (True, "accepted")
    assert _package_verdict(sb, N, mode, proof["bytes"], proof["roots"], proof["widths"], proof["raw_plan"], proof["values"]) is True


def _bump(element):
    limbs = element.limbs()
    return element.field.from_limbs([(limbs[0] + 1) % P, limbs[1], limbs[2] or 1])


AT = cases.START                                      # objects[AT]: points, AT + 1: shape, AT + 2: values, AT + 3: the quotient's root,
ROW = AT + 4                                          # then per index: (row, path) per commitment, the quotient's opening and its path


def _edit_value(objects):
    values = [[list(per_point) for per_point in per_group] for per_group in objects[AT + 2]]
    values[1][1][0] = _bump(values[1][1][0])
    return objects[:AT + 2] + [values] + objects[AT + 3:]


def _edit_second_row(objects):
    at = ROW + 2
    assert isinstance(objects[at], tuple) and len(objects[at]) == 9 and isinstance(objects[at + 1], list)
    row = list(objects[at])
    row[3] = _bump(row[3])
    return objects[:at] + [tuple(row)] + objects[at + 1:]


def _edit_shape(objects):
    widths, groups = objects[AT + 1]
    groups = list(groups)
    assert widths == (16, 9, 7) and groups[0][0][-1] == 18 and groups[1][0][-1] == 22
    groups[0], groups[1] = (groups[0][0][:-1], groups[0][1]), (tuple(sorted(groups[1][0] + (18,))), groups[1][1])
    return objects[:AT + 1] + [(widths, groups)] + objects[AT + 2:]


def _edit_widths_in_the_stream(objects):
    widths, groups = objects[AT + 1]
    return objects[:AT + 1] + [((15, 10, 7), groups)] + objects[AT + 2:]


def other_plans(plan):
    """the caller's plan changed three ways"""
    (c0, p0), (c1, p1), (c2, p2), (c3, p3) = plan
    moved = [(c0[:-1], p0), (sorted(c1 + c0[-1:]), p1), (c2, p2), (c3, p3)]
    swapped = [(c0, p1), (c1, p0), (c2, p2), (c3, p3)]
    changed = [(c0, [model.xadd(p0[0], (1, 0, 0)), p0[1]]), (c1, p1), (c2, p2), (c3, p3)]
    return {"moved": moved, "swapped": swapped, "changed": changed}


@pytest.mark.parametrize("N,mode", cases.PROTOCOL, ids=cases.PROTOCOL_IDS)
def test_the_verifier_refuses_tampered_streams_and_other_statements(sb, oracle, N, mode, capsys):
    proof = cases.model_proof(N, mode)
    data, roots, widths, plan, values = proof["bytes"], proof["roots"], proof["widths"], proof["raw_plan"], proof["values"]
    verdicts = {"untouched": _package_verdict(sb, N, mode, data, roots, widths, plan, values)}
    capsys.readouterr()
    refusals = {"value": dict(edit=_edit_value), "row of the second commitment": dict(edit=_edit_second_row), "shape": dict(edit=_edit_shape),
                "widths in the stream": dict(edit=_edit_widths_in_the_stream),
                "two roots swapped": dict(roots=[roots[1], roots[0], roots[2]]), "another root": dict(roots=[roots[0], bytes(64), roots[2]]),
                "a width moved": dict(widths=[15, 10, 7]), "a root too few": dict(roots=roots[:2]), "a width too few": dict(widths=[16, 16]),
                "five commitments": dict(roots=roots + roots[:2], widths=[16, 9, 5, 1, 1]), "a width of 0": dict(widths=[16, 16, 0]),
                "widths that are no numbers": dict(widths=[16, None, 7])}
    for name, other in other_plans(plan).items():
        refusals[name] = dict(plan=other)
    for name, change in refusals.items():
        verdicts[name] = _package_verdict(sb, N, mode, data, change.get("roots", roots), change.get("widths", widths), change.get("plan", plan), values,
                                          edit=change.get("edit"))
        printed = capsys.readouterr().out
        assert printed.count("\n") == 1, (name, printed)          # one line per refusal, and no exception
    assert verdicts == dict({name: False for name in refusals}, untouched=True)
    assert _model_verdict(sb, oracle, proof, roots=[roots[1], roots[0], roots[2]]) == (False, "row path")
    assert _model_verdict(sb, oracle, proof, widths=[15, 10, 7]) == (False, "widths")
    assert _model_verdict(sb, oracle, proof, roots=roots[:2]) == (False, "commitments")
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
    assert forced["roots"] == honest["roots"]
    assert _model_verdict(sb, oracle, forced)[0] is False
    capsys.readouterr()
    assert _package_verdict(sb, N, mode, forced["bytes"], forced["roots"], forced["widths"], forced["raw_plan"], forced["values"]) is False
    assert capsys.readouterr().out.count("\n") == 1


# ------------------------------------------------------------------------------------------------ 4. the plan's validation
def _commitments(*widths):
    return [types.SimpleNamespace(polys=[None] * w) for w in widths]          # (no commitment in HBM, no library call: refused first)


def test_bad_plans_and_bad_limits_are_refused_before_any_library_call(sb):
    from stark_brainfuck_amd import pcs
    N = 64
    pc = sb.PolynomialCommitment(_fri(sb, N, "default"))
    z = [(1 + i, 2, 3) for i in range(25)]
    omega = pc.xfield.modulus.coefficients[0].field.primitive_nth_root(N).value
    inside = (cases.OFFSET * pow(omega, 5, P) % P, 0, 0)
    three = _commitments(3, 2, 4)
    bad = {"overlapping groups": (three, [([0, 1, 2, 3, 4], [z[0]]), ([4, 5, 6, 7, 8], [z[1]])]),
           "a missing column": (three, [([0, 1, 2, 3], [z[0]]), ([5, 6, 7, 8], [z[1]])]),
           "a column too many": (three, [([0, 1, 2, 3, 4], [z[0]]), ([5, 6, 7, 8, 9], [z[1]])]),
           "descending columns": (three, [([1, 0, 2, 3, 4, 5, 6, 7, 8], [z[0]])]),
           "five points in a group": (three, [(list(range(9)), z[:5])]),
           "a domain point": (three, [(list(range(9)), [z[0], inside])]),
           "a point twice in one group": (three, [(list(range(9)), [z[1], (1 + 1 + P, 2, 3)])]),
           "no commitment": ([], [([0], [z[0]])]),
           "five commitments": (_commitments(1, 1, 1, 1, 1), [(list(range(5)), [z[0]])]),
           "a commitment of 33 columns": (_commitments(33), [(list(range(32)), [z[0]]), ([32], [z[0]])]),
           "25 groups": (_commitments(25), [([c], [z[0]]) for c in range(25)]),
           "49 pairs": (_commitments(13), [([c], z[:4]) for c in range(12)] + [([12], [z[0]])]),
           "25 points": (_commitments(25), [([2 * c, 2 * c + 1], [z[2 * c], z[2 * c + 1]]) for c in range(12)] + [([24], [z[24]])]),
           "a group of 33 columns": (_commitments(32, 2), [(list(range(33)), [z[0]]), ([33], [z[0]])]),
           "97 columns (by the plan)": (_commitments(32, 32, 32), [(list(range(32 * r, 32 * r + 32)), [z[0]]) for r in range(3)] + [([96], [z[0]])])}
    for name, (commitments, plan) in bad.items():
        ps = sb.ProofStream()
        with pytest.raises(ValueError):
            pc.open_rounds(commitments, plan, ps)
        assert ps.objects == [], name
    # the limits themselves are taken
    limit = cases.case("max", 64)["plan"]
    raw = [(columns, [limit.points[p] for p in indices]) for columns, indices in limit.groups]
    good = pc.rounds_plan(raw, [32, 32, 32])
    assert (good.m, len(good.groups), len(good.points), good.pairs) == (96, 24, 24, 48) and good.shape == limit.shape and good.base == limit.base
    # the wider limits are a parameter: a plan of one commitment keeps the old ones, with the old messages
    nine = [([c], [z[0]]) for c in range(9)]
    assert len(pcs.OpeningPlan(nine, pc.in_domain, 9, pcs.ROUNDS_LIMITS).groups) == 9
    with pytest.raises(ValueError, match="an opening plan has 1 .. 8 groups"):
        pcs.OpeningPlan(nine, pc.in_domain, 9)
    with pytest.raises(ValueError, match="an opening plan has 1 .. 8 groups"):
        pc.open_at(types.SimpleNamespace(polys=[None] * 9), nine, sb.ProofStream())
    with pytest.raises(ValueError, match="at most 32 columns"):
        pcs.OpeningPlan([(list(range(33)), [z[0]])], pc.in_domain)
    with pytest.raises(ValueError, match="at most 32 columns in a group"):
        pcs.OpeningPlan([(list(range(33)), [z[0]])], pc.in_domain, None, pcs.ROUNDS_LIMITS)


def test_global_column_numbers_the_columns_through(sb):
    pc = sb.PolynomialCommitment(_fri(sb, 64, "default"))
    commitments = _commitments(16, 9, 7)
    assert [pc.global_column(commitments, r, 0) for r in range(3)] == rmodel.first_columns([16, 9, 7]) == [0, 16, 25]
    assert pc.global_column(commitments, 2, 6) == rmodel.global_column([16, 9, 7], 2, 6) == 31 and pc.global_column([16, 9, 7], 1, 8) == 24
    for r, c in ((3, 0), (1, 9), (0, -1)):
        with pytest.raises(ValueError):
            pc.global_column(commitments, r, c)


def test_the_shape_goes_through_the_transcript_as_the_model_pushes_it(sb, oracle):
    """a tuple of a tuple of plain ints and a list of tuples of tuples: the same bytes from the package's stream and from the model's"""
    shape = ((16, 9, 7), [((0, 1, 18), (0, 1)), ((3, 22), (0, 2)), ((25,), (0,))])
    ps, ref = sb.ProofStream(), oracle.ProofStreamOracle()
    ps.push(shape)
    ref.push(shape)
    assert ps.serialize() == ref.serialize()
    assert sb.ProofStream().deserialize(ps.serialize()).pull() == shape
    proof = cases.model_proof(64, "default")
    assert proof["proof_stream"].objects[cases.START + 1] == (tuple(proof["widths"]), proof["plan"].shape)
