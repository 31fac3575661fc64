"""BrainfuckStark.prove_deep(zero_knowledge=True, secret_input=True) / verify_deep(...) on the MI355X ("Secret input"): the
proofs verify on an object that never saw the input, in both domain shapes and a non-default Fri mode; the constraint the mode drops is
the one that otherwise refuses them; two secrets prove one claim; other claims and every changed object are refused; the stream shows
nothing that is the secret's evaluation; the modes refuse each other; check_trace, check_air and the DEBUG degree check follow the same
rule; and the zero-knowledge mode without the switch keeps its bytes.  FRI domains here are 2^6 .. 2^11."""
import contextlib
import io
import os

import pytest

from tools import deep_stark_time as deep
from tools import stark_fri_modes as modes
from tools.stark_fri_modes import mode

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
SECRET = {"zero_knowledge": True, "secret_input": True}
# `,.` ("io") is the trace too short for the segmented zero-knowledge shape: there the refusal is expected, and the unsegmented proof made
CASES = [(name, mode(), segmented) for name in ("read2", "sum2", "plus1", "io") for segmented in (False, True)] + [
    ("read2", deep.MODE_A8C_G4, False), ("read2", deep.MODE_A8C_G4, True)]
IDS = ["%s%s%s" % (name, "" if m == mode() else "_a8c_g4", "_segmented" if segmented else "") for name, m, segmented in CASES]


@pytest.fixture(scope="module")
def sb():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import stark_brainfuck_amd
    return stark_brainfuck_amd


_made = {}


def proved(name, m=None, segmented=False, secret=None):
    """(stark, proof) of the secret-input claim on the seeded randomness with the intermediates kept, made once"""
    key = (name, modes.mode_id(m or mode()), segmented, secret)
    if key not in _made:
        _made[key] = deep.prove_secret_seeded(name, m, prepare=lambda s: setattr(s, "keep_intermediates", True), segmented=segmented, secret=secret)
    return _made[key]


def _golden(file):
    return open(os.path.join(GOLDEN, file), "rb").read()


def _refused(stark, proof, capsys, **kwargs):
    capsys.readouterr()
    verdict = stark.verify_deep(proof, **kwargs)
    printed = capsys.readouterr().out
    assert verdict is False and printed.count("\n") >= 1, (verdict, printed)
    return printed


# ------------------------------------------------------------------------------------------------ 1. accepts
@pytest.mark.parametrize("name,m,segmented", CASES, ids=IDS)
def test_a_verifier_without_the_input_accepts(sb, name, m, segmented):
    refusal = deep.secret_refusal(name, m, segmented)
    if refusal is not None:
        assert segmented and name == "io" and refusal == deep.zk_refusal(name, m, segmented)
        program, _, _, matrices = deep.secret_claim(name)
        with pytest.raises(ValueError) as raised:
            deep.make_secret_stark(name, m).prove_deep(program, *matrices, segmented=True, **SECRET)
        assert str(raised.value) == refusal
        segmented = False
    stark, proof = proved(name, m, segmented)
    shape = stark.deep_shape(segmented, True)
    assert shape.n <= 1 << 11 and (shape.fri.folding_factor, shape.fri.coset_leaves, shape.fri.grinding_bits) == (
        m["folding_factor"], m["coset_leaves"], m["grinding_bits"])
    verifier = deep.make_secret_stark(name, m)
    assert len(verifier.input_symbols) == 0 and verifier.input_table.height == 0
    assert verifier.verify_deep(proof, segmented=segmented, **SECRET) is True
    assert stark.input_table.height == 0 and stark._last["plan"].widths == (16, 9, shape.s + 1)
    assert tuple(stark._last["terminals"][2]) == (0, 0, 0)


def test_the_bytes_are_the_fixtures(sb):
    for name, m, segmented in deep.SECRET_FIXTURES:
        assert proved(name, m, segmented)[1] == _golden(deep.secret_fixture_file(name, m, segmented))


# ------------------------------------------------------------------------------------------------ 2. the constraint that is dropped
def test_without_the_switch_the_same_trace_is_refused_for_its_input_evaluation(sb, capsys):
    """the matrices of `,>,<.` run on "ab", the input matrix left empty as the claim's input table is: the zero-knowledge mode claims the
    EMPTY input, and its verifier refuses the processor's running input evaluation; with the switch the same matrices prove"""
    from stark_brainfuck_amd.vm import LazyTraceMatrix, VirtualMachine
    import numpy as np
    program, _, _, matrices = deep.secret_claim("read2", "ab")
    empty = LazyTraceMatrix(np.zeros((0, 1), dtype=np.uint64), VirtualMachine.field)
    given = list(matrices[:3]) + [empty, matrices[4]]
    stark, plain = deep.prove_secret_seeded("read2", secret_input=False, matrices=given)
    assert any(stark._last["terminals"][2])
    verifier = deep.make_secret_stark("read2")
    assert _refused(verifier, plain, capsys, zero_knowledge=True) == "a terminal does not match the public input, output or program\n"
    _, hidden = deep.prove_secret_seeded("read2", matrices=given)
    assert hidden == proved("read2")[1] and verifier.verify_deep(hidden, **SECRET) is True          # (the input matrix given reaches nothing)


# ------------------------------------------------------------------------------------------------ 3. the claim does not name the witness
def test_two_secrets_prove_the_same_claim(sb):
    verifier = deep.make_secret_stark("read2")
    proofs = [proved("read2", secret=secret)[1] for secret in ("ab", "ac")]
    assert proofs[0] != proofs[1]
    assert [verifier.verify_deep(proof, **SECRET) for proof in proofs] == [True, True]


# ------------------------------------------------------------------------------------------------ 4. soundness
@pytest.mark.parametrize("segmented", [False, True], ids=["unsegmented", "segmented"])
def test_other_claims_and_changed_objects_are_refused(sb, segmented, capsys):
    from stark_brainfuck_amd.vm import VirtualMachine
    stark, proof = proved("read2", segmented=segmented)
    kwargs = dict(SECRET, segmented=segmented)
    assert deep.make_secret_stark("read2").verify_deep(proof, **kwargs) is True
    # (the running time is stated through the processor table's padded height, as in every mode: 6 cycles and 7 are one claim, 9 another;
    # test_one_more_cycle_is_refused_where_it_is_another_claim has the `+ 1` that crosses a power of two)
    others = {"another output symbol": deep.make_secret_stark("read2", output_symbols=["b"]),
              "another program": deep.make_secret_stark("read2", program=VirtualMachine.compile(",>,>.")),
              "a running time of the next height": deep.make_secret_stark("read2", running_time=9)}
    assert others["a running time of the next height"].processor_table.height == 16 != stark.processor_table.height
    for what, verifier in others.items():
        _refused(verifier, proof, capsys, **kwargs)
    verifier = deep.make_secret_stark("read2")
    changed = deep.object_tamperings(proof)
    assert len(changed) == len(deep.objects_of(proof)) >= 30
    flipped = bytearray(proof)
    flipped[len(flipped) // 3] ^= 0x10
    changed.update({"a flipped byte": bytes(flipped), "a truncated proof": proof[:len(proof) // 2]})
    for what, data in changed.items():
        with contextlib.redirect_stdout(io.StringIO()) as out:
            verdict = verifier.verify_deep(data, **kwargs)
        assert verdict is False and out.getvalue().count("\n") >= 1, what
    # a false trace: the memory value the second read left (the second secret symbol) changed in the processor matrix alone
    import numpy as np
    from stark_brainfuck_amd.vm import LazyTraceMatrix
    program, _, _, matrices = deep.secret_claim("read2")
    values = np.array(matrices[0].values, dtype=np.uint64)
    values[3, 5] = (int(values[3, 5]) + 1) % ((1 << 64) - (1 << 32) + 1)
    false = [LazyTraceMatrix(np.ascontiguousarray(values), VirtualMachine.field)] + list(matrices[1:])
    false_proof = deep.prove_secret_seeded("read2", segmented=segmented, matrices=false)[1]
    _refused(verifier, false_proof, capsys, **kwargs)


def test_one_more_cycle_is_refused_where_it_is_another_claim(sb, capsys):
    """`+` runs 2 cycles; a verifier made for running_time + 1 = 3 has a processor table of height 4 and refuses the proof.  (Where
    running_time + 1 pads to the same height -- `,>,<.`: 6 and 7 -- the two objects state ONE claim and verify the same proofs, with
    or without secret_input: the protocol, like prove() and the reference, binds heights.)"""
    stark, proof = proved("plus1")
    own_time = deep.secret_claim("plus1")[1]
    assert own_time == 2 and deep.make_secret_stark("plus1").verify_deep(proof, **SECRET) is True
    _refused(deep.make_secret_stark("plus1", running_time=own_time + 1), proof, capsys, **SECRET)


# ------------------------------------------------------------------------------------------------ 5. what the stream shows
def _walk(obj):
    yield obj
    if isinstance(obj, (list, tuple)):
        for item in obj:
            yield from _walk(item)


@pytest.mark.parametrize("name", ["read2", "sum2"])
def test_nothing_in_the_stream_is_the_input_evaluation_terminal(sb, name):
    from stark_brainfuck_amd import air
    stark, proof = proved(name)
    gamma = tuple(int(v) for v in stark._last["challenges"][air.GAMMA])
    terminal = air.X0
    for symbol in deep.SECRET_PROGRAMS[name][1]:
        terminal = air.xadd(air.xmul(terminal, gamma), air.xlift(ord(symbol)))
    assert any(terminal) and tuple(stark.processor_table.input_evaluation_terminal) == terminal          # (the prover had it)
    objects = deep.objects_of(proof)
    seen = 0
    for o in (item for pushed in objects for item in _walk(pushed)):
        if hasattr(o, "limbs"):
            seen += 1
            assert tuple(v % air.P for v in o.limbs()) != terminal
        elif hasattr(o, "value"):
            seen += 1
            assert (o.value % air.P, 0, 0) != terminal
    assert seen > 30
    digests = [i for i, o in enumerate(objects[:8]) if isinstance(o, bytes) and len(o) == 64]
    assert digests[:3] == [0, 1, 6] and all(hasattr(o, "limbs") for o in objects[2:6]), "root0, root1, four terminals, root2"
    sent = [tuple(o.limbs()) for o in objects[2:6]]
    own = stark.get_terminals()
    assert sent == [tuple(own[i]) for i in (0, 1, 3, 4)]
    plan = stark._last["plan"]
    assert plan.table_group[3] is None and plan.empty_group is not None
    columns, points = plan.groups[plan.empty_group]
    assert columns == [14, 16 + 7] and len(points) == 1
    opened = stark._last["opened"][plan.empty_group]
    assert opened == [[(0, 0, 0), (0, 0, 0)]]
    assert [[tuple(v.limbs()) for v in per_point] for per_point in objects[9][plan.empty_group]] == opened


# ------------------------------------------------------------------------------------------------ 6. the modes refuse each other
def test_the_modes_refuse_each_others_proofs(sb, capsys):
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    program, running_time, outputs, matrices = deep.secret_claim("read2")
    public = BrainfuckStark(running_time, len(matrices[1]), program, list("ab"), outputs)          # the claim that states the input
    for segmented in (False, True):
        proof = proved("read2", segmented=segmented)[1]
        for verifier in (deep.make_secret_stark("read2"), public):
            for seg in (False, True):
                for zero_knowledge in (False, True):
                    _refused(verifier, proof, capsys, segmented=seg, zero_knowledge=zero_knowledge)
        _refused(deep.make_secret_stark("read2"), proof, capsys, segmented=not segmented, **SECRET)          # (the other domain shape)
    for name, m, segmented in deep.ZK_FIXTURES:
        if deep.zk_refusal(name, m, segmented) is None:
            _refused(deep.make_secret_stark(name, m), _golden(deep.zk_fixture_file(name, m, segmented)), capsys, segmented=segmented, **SECRET)


# ------------------------------------------------------------------------------------------------ 7. check_trace, check_air, DEBUG
def test_check_trace_leaves_out_the_two_checks_that_name_the_input(sb):
    from stark_brainfuck_amd.table import sample_ext
    stark = deep.make_secret_stark("read2")
    program, _, _, matrices = deep.secret_claim("read2")
    stream = modes.Stream(b"secret-check-trace")
    challenges = [sample_ext(stream(24)) for _ in range(11)]
    initials = [sample_ext(stream(24)) for _ in range(2)]
    assert stark.check_trace(*matrices) == []
    found = stark.check_trace(*matrices, challenges=challenges, initials=initials)
    assert [(v.table, v.kind, v.index) for v in found] == [("processor", "evaluation", 0)]          # the input is not the claim's (empty) one
    assert stark.check_trace(*matrices, challenges=challenges, initials=initials, secret_input=True) == []
    # an input matrix that is not what the processor read: reported without the switch, left out with it; everything else is still reported
    other = deep.secret_claim("read2", "zz")[3]
    given = list(matrices[:3]) + [other[3], matrices[4]]
    assert ("input", "evaluation", 0) in [(v.table, v.kind, v.index) for v in stark.check_trace(*given, challenges=challenges, initials=initials)]
    assert stark.check_trace(*given, challenges=challenges, initials=initials, secret_input=True) == []
    wrong_output = deep.make_secret_stark("read2", output_symbols=["b"])
    found = wrong_output.check_trace(*matrices, challenges=challenges, initials=initials, secret_input=True)
    assert [(v.table, v.kind, v.index) for v in found] == [("processor", "evaluation", 1)]


def test_check_air_and_the_debug_degree_check_pass_on_an_honest_secret_trace(sb, monkeypatch):
    monkeypatch.setenv("BFS_DEBUG", "1")
    for segmented in (False, True):
        stark, proof = deep.prove_secret_seeded("read2", prepare=lambda s: setattr(s, "check_air", True), segmented=segmented)
        assert proof == proved("read2", segmented=segmented)[1]


def test_the_debug_degree_check_fails_when_the_weight_is_kept(sb, monkeypatch):
    """the degree check sees the dropped constraint: with its weight kept and the terminal's slot zero the quotient is no polynomial"""
    from stark_brainfuck_amd import deep_stark
    monkeypatch.setenv("BFS_DEBUG", "1")
    monkeypatch.setattr(deep_stark, "secret_input_weights", lambda stark, weights: weights)
    with pytest.raises(AssertionError, match="degree >= S"):
        deep.prove_secret_seeded("read2")


# ------------------------------------------------------------------------------------------------ 8. the zero-knowledge mode untouched
def test_the_zero_knowledge_mode_without_the_switch_keeps_its_bytes(sb):
    assert deep.prove_deep_seeded("plus1", zero_knowledge=True)[1] == _golden("deep_zk_plus1_proof.bin")
    assert deep.prove_deep_seeded("two_io", zero_knowledge=True)[1] == _golden("deep_zk_two_io_proof.bin")
