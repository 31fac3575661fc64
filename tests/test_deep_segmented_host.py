"""The segmented mode of BrainfuckStark.prove_deep / verify_deep on the host, no GPU ("Segmented composition"): the domain
arithmetic of deep_segmented_shape(), the opening plan with s segments, an integer model of the split H(x) = sum_i x^(i L) H_i(x), and
verify_deep(segmented=True) on the committed proofs of tests/golden/deep_segmented.json (this project's own output on the MI355X,
tools/deep_stark_time.py --write-golden-segmented): accepted, their byte-level tamperings refused, each mode's proofs refused by the other."""
import hashlib
import os
import random

import pytest

from tools import deep_stark_time as deep
from tools.stark_fri_modes import mode

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
P = (1 << 64) - (1 << 32) + 1
CASES = [(name, mode()) for name in deep.PROGRAMS] + [("two_io", deep.MODE_A8C_G4)]
IDS = [deep.segmented_fixture_file(name, m)[len("deep_segmented_"):-len("_proof.bin")] for name, m in CASES]


@pytest.fixture(scope="session")
def sb():
    from stark_brainfuck_amd import build
    build.build_library()
    import stark_brainfuck_amd
    return stark_brainfuck_amd


# ------------------------------------------------------------------------------------------------ 1. domains
def _stark(sb, running_time, memory_length, program_length, log_expansion_factor=2):
    from stark_brainfuck_amd.algebra import BaseFieldElement
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    from stark_brainfuck_amd.vm import VirtualMachine
    program = [BaseFieldElement(0, VirtualMachine.field)] * program_length
    return BrainfuckStark(running_time, memory_length, program, [], [], log_expansion_factor, 2 * log_expansion_factor)


def _shape(sb, running_time, memory_length, program_length, log_expansion_factor=2):
    stark = _stark(sb, running_time, memory_length, program_length, log_expansion_factor)
    return stark, stark.deep_segmented_shape()


# (running time, memory length, program length) -> L, S, s, N today, N' = e L, W   at expansion factor 4
TABLE = {(2, 2, 10): (32, 256, 8, 1024, 128, 256),
         (19, 19, 10): (64, 512, 8, 2048, 256, 512),
         (1000, 600, 10): (2048, 16384, 8, 65536, 8192, 16384),
         (37254, 37254, 10): (1 << 17, 1 << 20, 8, 1 << 22, 1 << 19, 1 << 20)}


@pytest.mark.parametrize("claim", sorted(TABLE), ids=lambda c: "t%d_m%d_p%d" % c)
def test_the_domains_of_the_four_claims(sb, claim):
    stark, g = _shape(sb, *claim)
    L, S, s, N, n, w = TABLE[claim]
    assert (g.L, g.S, g.s, stark.fri.domain.length, g.n, g.w) == (L, S, s, N, n, w)
    # ... and as the definitions say: L holds the longest interpolant, S the composition polynomial, both domains lie in the working one
    longest = max(t.transform_coefficients() for t in stark.tables)
    assert L // 2 < longest <= L and S == max(stark.max_degree + 1, L) and s == S // L and n == stark.expansion_factor * L and w == max(n, S)
    assert (g.fri.domain.length, g.fri.domain.offset.value, g.fri.expansion_factor) == (n, stark.fri.domain.offset.value, stark.expansion_factor)
    assert g.fri.domain.omega.value == stark.field.primitive_nth_root(n).value
    assert (g.working_domain.length, g.working_domain.offset.value) == (w, g.domain.offset.value)
    assert pow(g.working_domain.omega.value, w // n, P) == g.domain.omega.value
    assert (g.fri.num_colinearity_tests, g.fri.folding_factor, g.fri.coset_leaves, g.fri.grinding_bits) == (stark.num_colinearity_checks, 2, False, 0)
    assert stark.deep_segmented_shape().fri is g.fri and stark.fri.domain.length == N          # made once, kept; the first Fri untouched
    # at expansion factor 16 the commitment domain is the working domain
    _, g16 = _shape(sb, *claim, log_expansion_factor=4)
    assert (g16.L, g16.S, g16.s, g16.n, g16.w) == (L, S, s, 16 * L, 16 * L) and g16.working_domain is g16.domain


@pytest.mark.parametrize("log_expansion_factor", [2, 4])
@pytest.mark.parametrize("claim", sorted(TABLE), ids=lambda c: "t%d_m%d_p%d" % c)
def test_the_unsegmented_shape_is_the_one_segment_case_on_the_first_fri(sb, claim, log_expansion_factor):
    from stark_brainfuck_amd.brainfuck_stark import deep_opening_plan
    stark = _stark(sb, *claim, log_expansion_factor=log_expansion_factor)
    g = stark.deep_shape(False)
    assert g.L == g.S == stark.max_degree + 1
    assert g.s == 1
    assert g.n == g.w == stark.fri.domain.length
    assert g.fri is stark.fri
    assert g.domain is g.working_domain is stark.fri.domain
    assert stark._segmented_fri == {}          # no second Fri was made
    assert vars(stark.deep_shape()) == vars(g)          # (the default is the unsegmented shape)
    numbers = lambda shape: (shape.L, shape.S, shape.s, shape.n, shape.w)
    again, named = stark.deep_shape(True), stark.deep_segmented_shape()
    (L, S, s), e = TABLE[claim][:3], 1 << log_expansion_factor
    assert numbers(again) == numbers(named) == (L, S, s, e * L, max(e * L, S))
    assert again.fri is named.fri and again.domain is named.domain is named.fri.domain and list(stark._segmented_fri) == [e * L]
    assert deep_opening_plan(stark.tables, (5, 6, 7), segments=g.s).widths[2] == 1


def test_the_unsegmented_shape_is_never_refused(sb, monkeypatch):
    stark, g = _shape(sb, 19, 19, 10)
    monkeypatch.setattr(stark, "max_degree", 32 * g.L - 1)
    one = stark.deep_shape(False)
    assert (one.L, one.S, one.s) == (32 * g.L, 32 * g.L, 1) and one.fri is stark.fri
    with pytest.raises(ValueError, match="segments"):
        stark.deep_shape(True)


FOUR_SEGMENTS = "+>+>+>" + "+" * 30 + "<<<+"          # 40 instructions whose memory trace has 142 rows: three cells are left and come back to


def test_the_forty_instruction_claim_has_four_segments(sb):
    """Running time 40 with a program of 40 instructions: the number of segments follows the rows of the MEMORY trace, which those two
    figures do not fix.  The instruction table has height 128 and a transition degree of 8 * 128 + 1, so S = 2048 whatever the memory
    table's height is; L is twice the tallest height.  A memory trace of 129 .. 256 rows (height 256, as the 40 instructions of
    FOUR_SEGMENTS have: the memory table holds a row for every cycle a cell waits to be visited again) gives L = 512 and s = 4,
    N' = W = 2048; one of at most 128 rows (as forty increments of one cell have) gives L = 256 and s = 8, N' = 1024, W = 2048."""
    for memory_length in (129, 142, 200, 256):
        stark, g = _shape(sb, 40, memory_length, 40)
        assert [t.height for t in stark.tables] == [64, 128, 256, 0, 0] and stark.max_degree + 1 == 2048
        assert (g.L, g.S, g.s, g.n, g.w) == (512, 2048, 4, 2048, 2048) and g.working_domain is g.domain
    for memory_length in (1, 40, 128):
        stark, g = _shape(sb, 40, memory_length, 40)
        assert stark.tables[1].height == 128 and stark.tables[2].height <= 128 and stark.max_degree + 1 == 2048
        assert (g.L, g.S, g.s, g.n, g.w) == (256, 2048, 8, 1024, 2048)
    # the two programs themselves
    program, running_time, _, _, matrices = deep.claim(FOUR_SEGMENTS)
    assert (len(program), running_time, len(matrices[1])) == (40, 41, 142)
    g = deep.make_stark(FOUR_SEGMENTS).deep_segmented_shape()
    assert (g.L, g.S, g.s, g.n, g.w) == (512, 2048, 4, 2048, 2048)
    program, running_time, _, _, matrices = deep.claim("+" * 40)
    assert (len(program), running_time) == (40, 41) and len(matrices[1]) <= 128
    g = deep.make_stark("+" * 40).deep_segmented_shape()
    assert (g.L, g.S, g.s, g.n, g.w) == (256, 2048, 8, 1024, 2048)


def test_the_fewest_segments_of_this_air_are_two(sb):
    """a memory table that dwarfs the others: its transition degree is 2 h + 1, L is 2 h"""
    stark, g = _shape(sb, 2, 5000, 10)
    assert [t.height for t in stark.tables] == [2, 16, 8192, 0, 0] and (g.L, g.S, g.s, g.n, g.w) == (16384, 32768, 2, 65536, 65536)


def test_more_than_sixteen_segments_are_refused(sb, monkeypatch):
    stark, g = _shape(sb, 19, 19, 10)
    monkeypatch.setattr(stark, "max_degree", 32 * g.L - 1)
    with pytest.raises(ValueError, match="segments"):
        stark.deep_segmented_shape()
    with pytest.raises(ValueError, match="segments"):
        stark.verify_deep(b"", segmented=True)


# ------------------------------------------------------------------------------------------------ 2. the plan
@pytest.mark.parametrize("segments", [1, 2, 8, 16])
def test_the_plan_with_segments(sb, segments):
    from stark_brainfuck_amd.brainfuck_stark import deep_opening_plan
    from stark_brainfuck_amd.pcs import ROUNDS_LIMITS, PolynomialCommitment
    z = (5, 6, 7)
    for name in deep.PROGRAMS:
        stark = deep.make_stark(name)
        today = deep_opening_plan(stark.tables, z)
        plan = deep_opening_plan(stark.tables, z, segments=segments)
        assert today.groups[-1] == ([25], [z]) and today.widths == (16, 9, 1)
        assert plan.groups[:-1] == today.groups[:-1] and plan.groups[-1] == (list(range(25, 25 + segments)), [z])
        assert plan.widths == (16, 9, segments)
        assert (plan.table_group, plan.empty_group, plan.h_group) == (today.table_group, today.empty_group, today.h_group)
        if segments == 1:
            assert vars(plan) == vars(today)
        checked = PolynomialCommitment(stark.deep_segmented_shape().fri).rounds_plan(plan.groups, list(plan.widths))
        assert checked.m == 25 + segments <= 25 + 16 and len(checked.groups) <= 7 and len(checked.points) <= 6 and checked.pairs <= 11
        assert max(len(columns) for columns, _ in plan.groups) <= 16 <= ROUNDS_LIMITS.group_columns


@pytest.mark.parametrize("segments", [0, 17, -1, 2.0, None])
def test_the_plan_refuses_other_segment_counts(sb, segments):
    from stark_brainfuck_amd.brainfuck_stark import deep_opening_plan
    with pytest.raises(ValueError, match="segments"):
        deep_opening_plan(deep.make_stark("io").tables, (5, 6, 7), segments=segments)


# ------------------------------------------------------------------------------------------------ 3. the split, on integers
@pytest.mark.parametrize("L", [1, 2, 8])
@pytest.mark.parametrize("s", [1, 2, 8])
def test_the_segments_at_z_recombine_to_the_polynomial_at_z(sb, L, s):
    from stark_brainfuck_amd import air
    rng = random.Random(1000 * L + s)
    triple = lambda: tuple(rng.randrange(P) for _ in range(3))
    S = L * s
    coefficients, z = [triple() for _ in range(S)], triple()

    def horner(cs, x):
        acc = air.X0
        for c in reversed(cs):
            acc = air.xadd(air.xmul(acc, x), c)
        return acc
    segments = [coefficients[i * L:(i + 1) * L] for i in range(s)]
    assert sum(len(f) for f in segments) == S and all(len(f) == L for f in segments)
    total = air.X0
    for i, f in enumerate(segments):
        total = air.xadd(total, air.xmul(air.xpow(z, i * L), horner(f, z)))
    assert total == horner(coefficients, z)
    # the verifier's form: Horner in z^L over the segments' values
    assert horner([horner(f, z) for f in segments], air.xpow(z, L)) == total


# ------------------------------------------------------------------------------------------------ 4. the fixtures
def _fixture(name, m):
    entry = next(e for e in deep.fixtures(listing=deep.SEGMENTED_FIXTURE_LIST) if e["file"] == deep.segmented_fixture_file(name, m))
    proof = open(os.path.join(GOLDEN, entry["file"]), "rb").read()
    assert hashlib.sha256(proof).hexdigest() == entry["proof_sha256"] and len(proof) == entry["proof_len"] and entry["args"] == m
    assert (entry["program"], entry["input"]) == deep.PROGRAMS[name] and entry["output"] == "".join(deep.claim(name)[3])
    assert entry["fri_domain_length"] == deep.SEGMENTED_DOMAINS[name]
    return proof


def test_the_fixture_list_names_the_five_segmented_proofs():
    listed = deep.fixtures(listing=deep.SEGMENTED_FIXTURE_LIST)
    assert sorted(e["file"] for e in listed) == sorted(["deep_segmented_plus1_proof.bin", "deep_segmented_io_proof.bin", "deep_segmented_two_io_proof.bin",
                                                        "deep_segmented_loop_proof.bin", "deep_segmented_two_io_a8c_g4_proof.bin"])
    assert all(os.path.getsize(os.path.join(GOLDEN, e["file"])) < (1 << 18) for e in listed)
    assert len(deep.fixtures()) == 5          # the unsegmented list is as it was


@pytest.mark.parametrize("name,m", CASES, ids=IDS)
def test_verify_deep_segmented_accepts_the_fixture_and_refuses_its_tamperings(sb, name, m, capsys):
    proof = _fixture(name, m)
    verifier = deep.make_stark(name, m)
    shape = verifier.deep_segmented_shape()
    assert shape.n == deep.SEGMENTED_DOMAINS[name] and shape.s == 8 and verifier.fri.domain.length == deep.DOMAINS[name]
    assert verifier.verify_deep(proof, segmented=True) is True
    assert capsys.readouterr().out == ""
    changed = dict(deep.tamperings(proof))
    changed.update(deep.segment_tamperings(proof))
    verdicts = {}
    for what, data in changed.items():
        assert data != proof
        verdicts[what] = verifier.verify_deep(data, segmented=True)
        assert capsys.readouterr().out.count("\n") == 1, what          # a refusal says why in one line, and nothing was raised
    assert verdicts == {what: False for what in verdicts} and len(verdicts) == 6
    # another claim: one more output symbol, another output symbol
    outputs = list(deep.claim(name)[3])
    others = [deep.make_stark(name, m, output_symbols=outputs + ["!"])]
    if outputs:
        others.append(deep.make_stark(name, m, output_symbols=[chr(ord(outputs[0]) ^ 1)] + outputs[1:]))
    assert [other.verify_deep(proof, segmented=True) for other in others] == [False] * len(others)
    # a proof of another FRI mode of the same claim
    other_mode = deep.MODE_A8C_G4 if m == mode() else mode(security_level=6)
    if not (name == "plus1" and other_mode == deep.MODE_A8C_G4):          # (32 points are too few for a fold by 8: that Fri refuses to be made)
        assert deep.make_stark(name, other_mode).verify_deep(proof, segmented=True) is False
    capsys.readouterr()
    # the other mode's verifier: False, one line, nothing raised
    assert verifier.verify_deep(proof) is False and verifier.verify_deep(proof, segmented=False) is False
    assert capsys.readouterr().out.count("\n") == 2
    # a proof of prove() of the same claim, and bytes that are no proof
    if name in ("plus1", "loop"):
        assert verifier.verify_deep(open(os.path.join(GOLDEN, "stark_%s_proof.bin" % name), "rb").read(), segmented=True) is False
    assert verifier.verify_deep(b"", segmented=True) is False and verifier.verify_deep(b"\x80\x04N.", segmented=True) is False
    assert verifier.verify_deep(proof, segmented=True) is True


@pytest.mark.parametrize("name,m", CASES, ids=IDS)
def test_the_unsegmented_fixtures_are_refused_by_the_segmented_verifier(sb, name, m, capsys):
    entry = next(e for e in deep.fixtures() if e["file"] == deep.fixture_file(name, m))
    proof = open(os.path.join(GOLDEN, entry["file"]), "rb").read()
    verifier = deep.make_stark(name, m)
    assert verifier.verify_deep(proof) is True
    assert capsys.readouterr().out == ""
    assert verifier.verify_deep(proof, segmented=True) is False
    assert capsys.readouterr().out.count("\n") == 1
