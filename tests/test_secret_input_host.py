"""prove_deep / verify_deep with secret_input=True without a GPU ("Secret input"): which weight the mode drops, from the
AIR's own lists; the two refusals of the arguments; and verify_deep(zero_knowledge=True, secret_input=True) on the committed proof --
its digest, the host identity of _verify_stream on its stream, what its objects show and do not show of the secret, every pushed object
changed, other claims, and the verifiers of the other modes against it and against theirs."""
import glob
import hashlib
import os

import numpy as np
import pytest

from tools import deep_stark_time as deep
from tools.stark_fri_modes import mode

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
SECRET = {"zero_knowledge": True, "secret_input": True}
ENTRIES = deep.fixtures(listing=deep.SECRET_FIXTURE_LIST)


def _golden(file):
    return open(os.path.join(GOLDEN, file), "rb").read()


def _refused(stark, proof, capsys, **kwargs):
    """-> the printed lines of a refusal: the verdict is False, something is printed, nothing is raised"""
    capsys.readouterr()
    verdict = stark.verify_deep(proof, **kwargs)
    printed = capsys.readouterr().out
    assert verdict is False and printed.count("\n") >= 1, (verdict, printed)
    return printed


# ------------------------------------------------------------------------------------------------ 1. the dropped weight
def test_the_dropped_weight_is_the_processors_input_evaluation_terminal_constraint():
    from stark_brainfuck_amd import air, deep_stark
    stark = deep.make_secret_stark("read2")
    processor = air.ProcessorAir()
    # counted from the AIR's own lists: the processor is the first table, its terminal constraints follow its boundary and transition ones
    assert stark.tables[0] is stark.processor_table
    before = len(processor.boundary()) + len(processor.transition())
    mine = [i for i, e in enumerate(processor.terminal())
            if e.op == "-" and (e.a.op, e.a.val) == ("t", 2) and (e.b.op, e.b.val) == ("v", (processor.IEV, False))]
    assert mine == [2] and before == 7 + 10
    at = deep_stark.dropped_weight(stark)
    assert at == before + mine[0] < stark.processor_table.num_quotients()
    kinds = [(t, kind, e) for t in stark.tables for kind, constraints in t.air.all() for e in constraints]
    assert len(kinds) + len(stark.permutation_arguments) == stark.deep_weight_count()
    assert kinds[at][0] is stark.processor_table and kinds[at][1] == "terminal" and kinds[at][2] is stark.processor_table.air.all()[2][1][2]
    # the same position whatever the claim
    assert {deep_stark.dropped_weight(deep.make_secret_stark(name)) for name in ("sum2", "plus1", "two_io")} == {at}


def test_only_that_weight_becomes_zero_in_a_copy():
    from stark_brainfuck_amd import deep_stark
    stark = deep.make_secret_stark("read2")
    count, at = stark.deep_weight_count(), deep_stark.dropped_weight(stark)
    array = np.arange(1, 3 * count + 1, dtype=np.uint64).reshape(count, 3)
    triples = [tuple(int(v) for v in row) for row in array]
    kept = array.copy()
    for given, out in ((array, deep_stark.secret_input_weights(stark, array)), (triples, deep_stark.secret_input_weights(stark, triples))):
        assert out is not given and len(out) == count
        assert [tuple(int(v) for v in w) for w in out] == triples[:at] + [(0, 0, 0)] + triples[at + 1:]
    assert (array == kept).all() and triples[at] != (0, 0, 0)
    assert deep_stark.sent_terminals(stark, False) == [0, 1, 2, 3, 4] and deep_stark.sent_terminals(stark, True) == [0, 1, 3, 4]


# ------------------------------------------------------------------------------------------------ 2. the arguments
def test_secret_input_on_a_claim_that_states_its_input_is_refused():
    program, _, _, _, matrices = deep.claim("two_io")
    public = deep.make_stark("two_io")
    assert len(public.input_symbols) == 2
    with pytest.raises(ValueError, match="input_symbols"):
        public.prove_deep(program, *matrices, **SECRET)
    with pytest.raises(ValueError, match="input_symbols"):
        public.verify_deep(b"", **SECRET)


def test_secret_input_without_zero_knowledge_is_refused():
    program, _, _, matrices = deep.secret_claim("read2")
    stark = deep.make_secret_stark("read2")
    for segmented in (False, True):
        with pytest.raises(ValueError, match="zero_knowledge=True"):
            stark.prove_deep(program, *matrices, segmented=segmented, secret_input=True)
        with pytest.raises(ValueError, match="zero_knowledge=True"):
            stark.verify_deep(b"", segmented=segmented, secret_input=True)


def test_the_claims_object_has_no_input_and_two_secrets_make_one_claim():
    a, b = deep.secret_claim("read2", "ab"), deep.secret_claim("read2", "ac")
    assert a[1:3] == b[1:3] and len(a[3][1]) == len(b[3][1]) and len(a[3][3]) == 2
    assert not np.array_equal(np.asarray(a[3][0].values), np.asarray(b[3][0].values))
    stark = deep.make_secret_stark("read2")
    assert stark.input_table.height == 0 and len(stark.input_symbols) == 0 and stark.output_symbols == ["a"]


# ------------------------------------------------------------------------------------------------ 3. the committed proof
def test_the_listing_names_the_fixture():
    assert [(e["name"], e["args"], e["segmented"]) for e in ENTRIES] == [(name, m, segmented) for name, m, segmented in deep.SECRET_FIXTURES]
    (e,) = ENTRIES
    assert e["file"] == "deep_zk_secret_two_io_proof.bin" == deep.secret_fixture_file("two_io", mode(), False)
    data = _golden(e["file"])
    assert len(data) == e["proof_len"] < (1 << 20) and hashlib.sha256(data).hexdigest() == e["proof_sha256"]
    assert (e["program"], e["secret"], e["output"]) == (",.,.", "ab", "ab") and e["fri_domain_length"] <= 1 << 11


def _proof():
    return _golden(ENTRIES[0]["file"])


def _walk(obj):
    yield obj
    if isinstance(obj, (list, tuple)):
        for item in obj:
            yield from _walk(item)


def test_verify_deep_accepts_the_committed_proof_and_the_host_identity_holds_on_its_stream():
    from stark_brainfuck_amd import deep_stark
    from stark_brainfuck_amd.ip import ProofStream
    verifier = deep.make_secret_stark("two_io")
    assert verifier.verify_deep(_proof(), **SECRET) is True
    shape = verifier.deep_shape(False, True)
    stream = ProofStream().deserialize(_proof())
    assert deep_stark._verify_stream(verifier, stream, shape, secret_input=True) is True
    assert stream.read_index == len(stream.objects)
    # ... and not with five terminals read, nor with the dropped weight kept
    assert deep_stark.verify(verifier, _proof(), shape) is False
    kept = deep_stark.secret_input_weights
    try:
        deep_stark.secret_input_weights = lambda stark, weights: weights
        assert deep_stark._verify_stream(verifier, ProofStream().deserialize(_proof()), shape, secret_input=True) is False
    finally:
        deep_stark.secret_input_weights = kept


def test_the_stream_holds_four_terminals_and_nothing_that_is_the_secrets_evaluation():
    from stark_brainfuck_amd import air, deep_stark
    from stark_brainfuck_amd.ip import ProofStream
    verifier = deep.make_secret_stark("two_io")
    stream = ProofStream().deserialize(_proof())
    objects = list(stream.objects)
    digests = [i for i, o in enumerate(objects[:8]) if isinstance(o, bytes) and len(o) == 64]
    assert digests[:3] == [0, 1, 6], "root0, root1, four terminals, root2"
    assert all(hasattr(o, "limbs") for o in objects[2:6])
    stream.pull()
    challenges = type(verifier)._sample_weights(11, stream.verifier_fiat_shamir())
    gamma = tuple(challenges[air.GAMMA])
    terminal = air.X0
    for symbol in ENTRIES[0]["secret"]:          # sum symbol_i gamma^(n - i), in Python ints
        terminal = air.xadd(air.xmul(terminal, gamma), air.xlift(ord(symbol)))
    assert any(terminal[1:]), "the evaluation of two symbols in an extension-field challenge is no base-field element"
    seen = 0
    for o in (item for pushed in objects for item in _walk(pushed)):
        if hasattr(o, "limbs"):
            seen += 1
            assert tuple(v % air.P for v in o.limbs()) != terminal
        elif hasattr(o, "value"):
            seen += 1
            assert (o.value % air.P, 0, 0) != terminal
    assert seen > 30
    # the public-input proof of the same program does show it, at index 4 of its stream (what this mode takes out)
    public = list(ProofStream().deserialize(_golden("deep_zk_two_io_proof.bin")).objects)
    public_stream = ProofStream().deserialize(_golden("deep_zk_two_io_proof.bin"))
    public_stream.pull()
    g = tuple(type(verifier)._sample_weights(11, public_stream.verifier_fiat_shamir())[air.GAMMA])
    assert tuple(public[4].limbs()) == air.xadd(air.xmul(air.xlift(ord("a")), g), air.xlift(ord("b")))
    # the input table's columns: in the plan's group of tables without rows, opened as zeros
    values_at = 9
    z = tuple(objects[values_at - 2][0].limbs())
    plan = deep_stark.deep_opening_plan(verifier.tables, z, segments=1, randomizer=True)
    assert plan.table_group[3] is None and plan.empty_group is not None
    columns, points = plan.groups[plan.empty_group]
    assert columns == [14, 16 + 7] and len(points) == 1          # the input table's base column and its extension column
    opened = objects[values_at][plan.empty_group]
    assert len(opened) == 1 and len(opened[0]) == 2 and all(tuple(v.limbs()) == (0, 0, 0) for v in opened[0])


def test_every_pushed_object_changed_is_refused():
    verifier = deep.make_secret_stark("two_io")
    changed = deep.object_tamperings(_proof())
    assert len(changed) == len(deep.objects_of(_proof())) >= 40
    import contextlib
    import io
    for what, data in changed.items():
        assert data != _proof()
        with contextlib.redirect_stdout(io.StringIO()) as out:
            verdict = verifier.verify_deep(data, **SECRET)
        assert verdict is False and out.getvalue().count("\n") >= 1, what
    flipped = bytearray(_proof())
    flipped[len(flipped) // 3] ^= 0x10
    with contextlib.redirect_stdout(io.StringIO()):
        assert verifier.verify_deep(bytes(flipped), **SECRET) is False
        assert verifier.verify_deep(_proof()[:len(_proof()) // 2], **SECRET) is False
    assert verifier.verify_deep(_proof(), **SECRET) is True


def test_another_output_another_program_and_another_running_time_are_refused(capsys):
    """A claim states its running time through the processor table's PADDED height (Table: the power of two >= running_time; the
    padding rows keep counting cycles), in this protocol as in prove() and the reference: 5 cycles and 6 are one claim, and a verifier
    made for 6 accepts this proof with or without secret_input.  What is refused is a running time of another height -- here 9 cycles;
    test_gpu_secret_input.py has `+`, whose 2 cycles plus one cross a power of two."""
    from stark_brainfuck_amd.vm import VirtualMachine
    own_time = deep.secret_claim("two_io")[1]
    assert own_time == 5 and deep.make_secret_stark("two_io", running_time=9).processor_table.height == 16 != deep.make_secret_stark("two_io").processor_table.height
    others = {"another output symbol": deep.make_secret_stark("two_io", output_symbols=["a", "c"]),
              "one output symbol fewer": deep.make_secret_stark("two_io", output_symbols=["a"]),
              "another program": deep.make_secret_stark("two_io", program=VirtualMachine.compile(",.,+")),
              "a running time of the next height": deep.make_secret_stark("two_io", running_time=9)}
    for what, verifier in others.items():
        _refused(verifier, _proof(), capsys, **SECRET)
    assert "terminal does not match" in _refused(others["another output symbol"], _proof(), capsys, **SECRET)
    assert "terminal does not match" in _refused(others["another program"], _proof(), capsys, **SECRET)


def test_the_modes_refuse_each_others_proofs(capsys):
    """the four verifiers without secret_input against the secret-input proof -- on the object without the input and on the one that
    states it --, and the secret-input verifier against every committed zero-knowledge proof, on its claim without the input"""
    for verifier in (deep.make_secret_stark("two_io"), deep.make_stark("two_io")):
        for segmented in (False, True):
            for zero_knowledge in (False, True):
                _refused(verifier, _proof(), capsys, segmented=segmented, zero_knowledge=zero_knowledge)
    files = sorted(os.path.basename(f) for f in glob.glob(os.path.join(GOLDEN, "deep_zk_*_proof.bin")) if "deep_zk_secret_" not in f)
    listed = {e["file"]: e for e in deep.fixtures(listing=deep.ZK_FIXTURE_LIST) if e["file"]}
    assert files == sorted(listed) and len(files) == 9
    for file, e in listed.items():
        verifier = deep.make_secret_stark(e["name"], e["args"])
        assert len(verifier.input_symbols) == 0
        _refused(verifier, _golden(file), capsys, segmented=e["segmented"], **SECRET)
        if not deep.PROGRAMS[e["name"]][1]:          # (a claim that reads nothing: the plain zero-knowledge verifier on the same object accepts)
            assert verifier.verify_deep(_golden(file), segmented=e["segmented"], zero_knowledge=True) is True
