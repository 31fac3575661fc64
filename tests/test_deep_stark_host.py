"""BrainfuckStark.verify_deep, the opening plan of the mode and PolynomialCommitment.read_rounds on the host, no GPU: the committed
proofs of tests/golden/deep_stark.json (this project's own output on the MI355X, tools/deep_stark_time.py --write-golden) are accepted and
their byte-level tamperings refused; the plan builder gives the groups of the four height patterns; read_rounds agrees with verify_rounds on
the CPython model's opening (tests/pcs_rounds_model.py)."""
import hashlib
import os

import pytest

import pcs_rounds_cases as cases
from tools import deep_stark_time as deep
from tools.stark_fri_modes import mode

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
CASES = [(name, mode()) for name in deep.PROGRAMS] + [("two_io", deep.MODE_A8C_G4)]
IDS = [deep.fixture_file(name, m)[len("deep_"):-len("_proof.bin")] for name, m in CASES]


@pytest.fixture(scope="session")
def sb():
    from stark_brainfuck_amd import build
    build.build_library()
    import stark_brainfuck_amd
    return stark_brainfuck_amd


def _fixture(name, m):
    entry = next(e for e in deep.fixtures() if e["file"] == deep.fixture_file(name, m))
    proof = open(os.path.join(GOLDEN, entry["file"]), "rb").read()
    assert hashlib.sha256(proof).hexdigest() == entry["proof_sha256"] and len(proof) == entry["proof_len"] and entry["args"] == m
    assert (entry["program"], entry["input"]) == deep.PROGRAMS[name] and entry["output"] == "".join(deep.claim(name)[3])
    return proof


def test_the_fixture_list_names_the_five_proofs():
    assert sorted(e["file"] for e in deep.fixtures()) == sorted(["deep_plus1_proof.bin", "deep_io_proof.bin", "deep_two_io_proof.bin", "deep_loop_proof.bin",
                                                                 "deep_two_io_a8c_g4_proof.bin"])
    assert all(os.path.getsize(os.path.join(GOLDEN, e["file"])) < (1 << 18) for e in deep.fixtures())


@pytest.mark.parametrize("name,m", CASES, ids=IDS)
def test_verify_deep_accepts_the_fixture_and_refuses_its_tamperings(sb, name, m, capsys):
    proof = _fixture(name, m)
    verifier = deep.make_stark(name, m)
    assert verifier.fri.domain.length == deep.DOMAINS[name]
    assert verifier.verify_deep(proof) is True
    assert capsys.readouterr().out == ""
    verdicts = {}
    for what, data in deep.tamperings(proof).items():
        assert data != proof
        verdicts[what] = verifier.verify_deep(data)
        assert capsys.readouterr().out.count("\n") == 1, what          # a refusal says why in one line, and nothing was raised
    assert verdicts == {what: False for what in verdicts} and len(verdicts) == 4
    # another claim: one more output symbol, another output symbol, another input symbol
    outputs = list(deep.claim(name)[3])
    others = [deep.make_stark(name, m, output_symbols=outputs + ["!"])]
    if outputs:
        others.append(deep.make_stark(name, m, output_symbols=[chr(ord(outputs[0]) ^ 1)] + outputs[1:]))
    assert [other.verify_deep(proof) for other in others] == [False] * len(others)
    # a proof of another mode of the same claim
    other_mode = deep.MODE_A8C_G4 if m == mode() else mode(security_level=6)
    assert deep.make_stark(name, other_mode).verify_deep(proof) is False
    capsys.readouterr()
    # a proof of prove() of the same claim, and bytes that are no proof
    if name in ("plus1", "loop"):
        assert verifier.verify_deep(open(os.path.join(GOLDEN, "stark_%s_proof.bin" % name), "rb").read()) is False
    assert verifier.verify_deep(b"") is False and verifier.verify_deep(b"\x80\x04N.") is False
    assert verifier.verify_deep(proof) is True


def test_the_plan_builder_gives_the_groups_of_the_four_height_patterns(sb):
    from stark_brainfuck_amd.air import xscale
    from stark_brainfuck_amd.brainfuck_stark import deep_opening_plan
    from stark_brainfuck_amd.pcs import PolynomialCommitment
    z = (5, 6, 7)
    processor, instruction, memory = list(range(0, 7)) + list(range(16, 20)), [7, 8, 9, 20, 21], [10, 11, 12, 13, 22]
    expected = {"plus1": ([processor, instruction, memory, [14, 15, 23, 24], [25]], [2, 2, 1, 1, 1], [0, 1, 2, None, None], 3),
                "io": ([processor, instruction, memory, [14, 23], [15, 24], [25]], [2, 2, 2, 1, 1, 1], [0, 1, 2, 3, 4], None),
                "two_io": ([processor, instruction, memory, [14, 23], [15, 24], [25]], [2, 2, 2, 2, 2, 1], [0, 1, 2, 3, 4], None),
                "loop": ([processor, instruction, memory, [15, 24], [14, 23], [25]], [2, 2, 2, 1, 1, 1], [0, 1, 2, None, 3], 4)}
    shapes = {}
    for name, (columns, points, table_group, empty_group) in expected.items():
        stark = deep.make_stark(name)
        assert (stark.input_table.height, stark.output_table.height) == deep.HEIGHTS[name]
        plan = deep_opening_plan(stark.tables, z)
        assert [c for c, _ in plan.groups] == columns and [len(p) for _, p in plan.groups] == points
        assert (plan.widths, plan.table_group, plan.empty_group, plan.h_group) == ((16, 9, 1), table_group, empty_group, len(columns) - 1)
        for t, g in zip(stark.tables, table_group):
            if g is not None:          # height 1: the row itself is its next row, one point; else z and z times the subgroup generator
                assert plan.groups[g][1] == ([z] if t.height == 1 else [z, xscale(z, t.omicron.value)]) and (t.height != 1 or t.omicron.value == 1)
        assert all(p == [z] for _, p in plan.groups[len([g for g in table_group if g is not None]):])
        checked = PolynomialCommitment(stark.fri).rounds_plan(plan.groups, list(plan.widths))          # within open_rounds' limits, every column once
        shapes[name] = (len(checked.groups), len(checked.points), checked.pairs)
        assert checked.m == 26
    # (the memory table of "+" has one row; instruction and memory table of the loop share a height, hence a point)
    assert shapes == {"plus1": (5, 3, 7), "io": (6, 4, 9), "two_io": (6, 5, 11), "loop": (6, 3, 9)}
    assert all(g <= 7 and p <= 6 and pairs <= 11 for g, p, pairs in shapes.values())


@pytest.mark.parametrize("N,mode_name", cases.PROTOCOL, ids=cases.PROTOCOL_IDS)
def test_read_rounds_agrees_with_verify_rounds_on_the_models_opening(sb, N, mode_name, capsys):
    import test_pcs_rounds_host as host
    proof = cases.model_proof(N, mode_name)
    data, roots, widths, plan = proof["bytes"], proof["roots"], proof["widths"], proof["raw_plan"]
    pc = sb.PolynomialCommitment(host._fri(sb, N, mode_name))

    def read(edit=None, **other):
        ps = sb.ProofStream().deserialize(data)
        if edit is not None:
            ps.objects = edit(list(ps.objects))
        for _ in range(cases.START):
            ps.pull()
        return pc.read_rounds(other.get("roots", roots), other.get("widths", widths), other.get("plan", plan), ps)
    values = read()
    assert capsys.readouterr().out == ""
    assert values == [[[tuple(v) for v in per_point] for per_point in per_group] for per_group in proof["values"]]
    assert host._package_verdict(sb, N, mode_name, data, roots, widths, plan, values) is True          # what it returns makes verify_rounds accept
    # a changed value in the stream: neither accepts (verify_rounds is asked with the changed value, so that it too gets as far as the quotient)
    capsys.readouterr()
    assert read(edit=host._edit_value) is None
    assert capsys.readouterr().out.count("\n") == 1
    changed = [[list(per_point) for per_point in per_group] for per_group in values]
    changed[1][1][0] = ((changed[1][1][0][0] + 1) % host.P, changed[1][1][0][1], changed[1][1][0][2] or 1)
    assert host._package_verdict(sb, N, mode_name, data, roots, widths, plan, changed, edit=host._edit_value) is False
    # what verify_rounds refuses about the statement, read_rounds refuses too: None, one line, no exception
    refusals = {"a shape of other groups": dict(edit=host._edit_shape), "another root": dict(roots=[roots[0], bytes(64), roots[2]]), "a width moved": dict(widths=[15, 10, 7]),
                "a root too few": dict(roots=roots[:2]), "a row of the second commitment": dict(edit=host._edit_second_row)}
    for name, other in host.other_plans(plan).items():
        refusals[name] = dict(plan=other)
    for name, change in refusals.items():
        capsys.readouterr()
        assert read(**change) is None, name
        assert capsys.readouterr().out.count("\n") == 1, name


def test_read_rounds_refuses_values_of_another_shape_or_not_canonical(sb, capsys):
    import test_pcs_rounds_host as host
    N, mode_name = cases.PROTOCOL[0]
    proof = cases.model_proof(N, mode_name)
    pc = sb.PolynomialCommitment(host._fri(sb, N, mode_name))
    AT = cases.START + 2

    def read(edit):
        ps = sb.ProofStream().deserialize(proof["bytes"])
        ps.objects = edit(list(ps.objects))
        for _ in range(cases.START):
            ps.pull()
        return pc.read_rounds(proof["roots"], proof["widths"], proof["raw_plan"], ps)

    def with_values(change):
        def edit(objects):
            values = [[list(per_point) for per_point in per_group] for per_group in objects[AT]]
            return objects[:AT] + [change(values)] + objects[AT + 1:]
        return edit

    def unreduced(values):
        limbs = values[0][0][0].limbs()
        values[0][0][0] = values[0][0][0].field.from_limbs([limbs[0] + host.P, limbs[1], limbs[2]])
        return values
    edits = {"a value too few": with_values(lambda v: [v[0][:1] + [v[0][1][:-1]]] + v[1:]), "a group too few": with_values(lambda v: v[:-1]),
             "an int for a value": with_values(lambda v: [[[5] + v[0][0][1:]] + v[0][1:]] + v[1:]), "no list": with_values(lambda v: None),
             "an unreduced limb": with_values(unreduced)}
    for name, edit in edits.items():
        capsys.readouterr()
        assert read(edit) is None, name
        assert capsys.readouterr().out.count("\n") == 1, name
