"""BrainfuckStark(..., folding_factor, coset_leaves, grinding_bits) on the GPU ("FRI modes at the STARK level"): the stream
from the combination root on against `oracle` and the three FRI models, the two stage drivers against each other and against the
committed fixtures, both verifier routes, proof sizes, and the default mode against the reference's own proofs.

The domains are 2^8 ("+") and 2^11 ("++[>+<-]>."): with folding by 8 the first has two codewords and one layer -- the smallest shape
that still folds -- the second three, the smallest where one coset layer hands `expected` to the next; folding by 4 gives five."""
import glob
import hashlib
import json
import os
import pickle
from hashlib import blake2b

import pytest

import fri_coset_model
import fri_grinding_model
import stark_fri_modes_streams as streams
from soundness_cases import ACCEPTED, outcome
from tools import stark_fri_modes as modes
from tools.stark_fri_modes import mode

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
NAMES = sorted(os.path.basename(p)[len("stark_"):-len(".json")] for p in glob.glob(os.path.join(GOLDEN, "stark_*.json")))

MODES = [mode(4), mode(8), mode(2, True), mode(4, True), mode(8, True), mode(8, True, 5, security_level=7), mode(2, False, 3, security_level=5)]
# (the two grinding modes keep t = (security_level - bits) // 2 = 1 colinearity check, like the modes without grinding)
CASES = [("loop", m) for m in MODES] + [("plus1", mode(8, True))]
IDS = ["%s-%s" % (name, modes.mode_id(m)) for name, m in CASES]

_proofs = {}


def proofs_of(name, m):
    """the proof of golden program `name` in mode m on the golden's randomness, by every route, made once:
    native: the native stage driver (bfs_stark_commit / bfs_stark_finish);  python: the Python stage driver, openings through
    bfs_stark_push_openings(_cosets);  objects: the Python stage driver with the openings made of Python objects (_openings_python);
    kept: the Python stage driver with keep_intermediates, into a proof stream of the test's -- with the stark, for its `_last`"""
    from stark_brainfuck_amd import ProofStream
    key = (name, modes.mode_id(m))
    if key not in _proofs:
        def python_driver(s):
            s.native_stages = False

        def python_objects(s):
            s.native_stages = False
            s._openings_native = lambda p: None

        def keep(s):
            s.keep_intermediates = True
        out = {"native": modes.prove_seeded(name, m)[1], "python": modes.prove_seeded(name, m, prepare=python_driver)[1],
               "objects": modes.prove_seeded(name, m, prepare=python_objects)[1]}
        stream = ProofStream()
        out["stark"], out["kept"] = modes.prove_seeded(name, m, prepare=keep, proof_stream=stream)
        out["stream"] = stream
        _proofs[key] = out
    return _proofs[key]


@pytest.mark.parametrize("name,m", CASES, ids=IDS)
def test_stream_from_the_combination_root_on_is_the_models(name, m):
    """the combination codeword read back from HBM; from it, with `oracle` and the models alone: the root, the indices, the openings
    of the combination as DESIGN.md defines them, FRI (fri_grinding_model.prove over the stream so far).  What lies between the root
    and the combination openings -- the opened ROWS, which no mode changes -- is taken from the proof itself; the verifier tests and
    the default-mode goldens cover it."""
    from oracle import ref_oracle as o
    made = proofs_of(name, m)
    stark, proof = made["stark"], made["kept"]
    n, a, coset = stark.fri.domain.length, m["folding_factor"], m["coset_leaves"]
    cw = stark._last["combination"].to_numpy()
    assert cw.shape == (3, n)
    by_value = lambda x: streams.by_value(o, x)
    actual = streams.load(o, proof)       # (the oracle's look-alike classes, on the oracle's own field objects)
    assert [by_value(x) for x in actual] == [by_value(x) for x in made["stream"].objects]
    # ---- everything before the combination root is the default-mode proof's for the same seed
    ROOT_AT = 7                           # base root, extension root, five terminals
    golden = streams.load(o, open(os.path.join(GOLDEN, "stark_%s_proof.bin" % name), "rb").read())
    assert o.dumps(actual[:ROOT_AT]) == o.dumps(golden[:ROOT_AT])
    # ---- the root
    expected = o.ProofStreamOracle()
    expected.objects = list(actual[:ROOT_AT])
    if coset:
        tree, leaves, _ = fri_coset_model.coset_merkle(o, cw, a)
        q = n // a
    else:
        tree, leaves = o.xfe_merkle(cw)
        q = n
    assert tree.num_leafs == q
    expected.push(tree.root())
    assert stark._last["combination_tree"].root() == tree.root()
    # ---- the indices, the rows (taken over), the openings of the combination
    seed = expected.prover_fiat_shamir()
    indices = [int.from_bytes(blake2b(seed + bytes(i)).digest(), "big") % n for i in range(m["security_level"])]
    assert indices == stark._last["indices"]
    rows = m["security_level"] * (1 + len(stark._layout.unit_distances(n))) * 4
    expected.objects += actual[ROOT_AT + 1:ROOT_AT + 1 + rows]
    for i in indices:
        expected.push(leaves[i % q])          # coset: the tuple of the elements at c + j q, c = i mod q; else the element at i
        expected.push(tree.open(i % q))
        assert len(expected.objects[-1]) == q.bit_length() - 1
        if coset:
            assert len(leaves[i % q]) == a and by_value(leaves[i % q][i // q]) == ("xfe", tuple(int(v) for v in cw[:, i]))
    # ---- FRI over the stream so far
    ref = fri_grinding_model.prove(o, cw, stark.fri.domain.offset.value, stark.fri.domain.omega.value, stark.expansion_factor,
                                   stark.num_colinearity_checks, a, coset, m["grinding_bits"], proof_stream=expected)
    want = ref["proof_stream"].objects
    assert (ref["nonce"] is not None) == bool(m["grinding_bits"])
    assert len(actual) == len(want)
    for k, (got, exp) in enumerate(zip(actual, want)):
        assert by_value(got) == by_value(exp), "object %d of %d" % (k, len(want))
    if m["grinding_bits"]:
        at = ROOT_AT + 1 + rows + 2 * len(indices) + ref["rounds"]          # roots of rounds 1.., the last codeword, then the nonce
        assert type(actual[at]) is int and actual[at] == ref["nonce"]
    assert ref["rounds"] == stark.fri.num_rounds() == {("loop", 8): 3, ("loop", 4): 5, ("loop", 2): 9, ("plus1", 8): 2}[(name, a)]


@pytest.mark.parametrize("name,m", CASES, ids=IDS)
def test_the_stage_drivers_write_identical_bytes(name, m):
    """object identity included: the bytes are pickle's, which writes a back-reference for an object it has seen"""
    made = proofs_of(name, m)
    assert made["native"] == made["python"], "native stage driver against the Python stage driver"
    assert made["native"] == made["objects"], "openings pushed natively against openings made of Python objects"
    assert made["native"] == made["kept"], "against the Python stage driver with the quotients written out"
    for entry in modes.fixtures():
        if entry["name"] == name and entry["args"] == m:
            committed = open(os.path.join(GOLDEN, entry["file"]), "rb").read()
            assert hashlib.sha256(committed).hexdigest() == entry["proof_sha256"]
            assert made["native"] == committed, entry["file"]


def test_every_fixture_mode_is_proven_here():
    """the committed fixtures are modes this file proves, or proves below (the grinding ones with security_level 2)"""
    listed = modes.fixtures()
    assert sorted((e["name"], modes.mode_id(e["args"])) for e in listed) == sorted((name, modes.mode_id(m)) for name, m in modes.FIXTURES)
    for entry in listed:
        proof = modes.prove_seeded(entry["name"], entry["args"])[1]
        assert hashlib.sha256(proof).hexdigest() == entry["proof_sha256"], entry["file"]
        assert proof == open(os.path.join(GOLDEN, entry["file"]), "rb").read()
        assert proof == modes.prove_seeded(entry["name"], entry["args"], prepare=lambda s: setattr(s, "native_stages", False))[1]


@pytest.mark.parametrize("name,m", CASES, ids=IDS)
def test_both_verifier_routes_accept(name, m):
    proof = proofs_of(name, m)["native"]
    args = modes.stark_args(modes.PROGRAMS[name], m)
    for native in (True, False):
        assert outcome(args, proof, native) == ACCEPTED, "native" if native else "python"


@pytest.mark.parametrize("name,m", CASES, ids=IDS)
def test_the_native_verifier_decides_itself(name, m):
    """True, not None: no mode is handed to the Python verifier"""
    assert modes.make_stark(modes.PROGRAMS[name], m)._verify_native(proofs_of(name, m)["native"]) is True


def test_coset_leaves_make_the_proof_smaller():
    """by counting, on the 2^11 domain with t = 1.  The default FRI has nine codewords of 2^11 .. 2^3 elements; layer r < 7 opens two
    paths of 11 - r digests and one of 10 - r, the last layer two of 4: 112 + 49 + 8 = 169.  Folding by 8 over cosets has three
    codewords, 2^11, 2^8, 2^5, and one path per layer into trees of 2^8 and 2^5 leaves: 8 + 5 = 13.  Each of the two combination paths
    has 8 digests instead of 11; the opened rows have as many digests in either mode."""
    default = modes.prove_seeded("loop", mode())[1]
    assert default == open(os.path.join(GOLDEN, "stark_loop_proof.bin"), "rb").read()
    folded = proofs_of("loop", mode(8, True))["native"]
    assert len(folded) < len(default)
    assert modes.count_digests(default) - modes.count_digests(folded) == (169 - 13) + 2 * (11 - 8)
    # ... and with grinding: two bits at security level 4 leave one colinearity check instead of two
    plain4 = modes.prove_seeded("loop", mode(security_level=4))
    coset4 = modes.prove_seeded("loop", mode(8, True, security_level=4))
    ground4 = modes.prove_seeded("loop", mode(8, True, 2, security_level=4))
    assert (plain4[0].num_colinearity_checks, coset4[0].num_colinearity_checks, ground4[0].num_colinearity_checks) == (2, 2, 1)
    assert len(ground4[1]) < len(coset4[1]) < len(plain4[1])
    assert modes.count_digests(coset4[1]) - modes.count_digests(ground4[1]) == 13
    for stark, proof in (plain4, coset4, ground4):
        assert stark.verify(proof) is True


@pytest.mark.parametrize("name", NAMES)
def test_default_arguments_written_out_give_the_reference_proof(name, monkeypatch):
    from stark_brainfuck_amd import brainfuck_stark, salted_merkle, table
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    from stark_brainfuck_amd.vm import VirtualMachine
    g = json.load(open(os.path.join(GOLDEN, "stark_%s.json" % name)))
    program = VirtualMachine.compile(g["program"])
    running_time, input_symbols, output_symbols = VirtualMachine.run(program, input_data=list(g["input"]))
    matrices = VirtualMachine.simulate(program, input_data=list(input_symbols))
    stark = BrainfuckStark(running_time, len(matrices[1]), program, input_symbols, output_symbols, log_expansion_factor=2, security_level=2,
                           folding_factor=2, coset_leaves=False, grinding_bits=0)
    stream = modes.Stream(name.encode())
    for mod in (brainfuck_stark, salted_merkle, table):
        monkeypatch.setattr(mod, "urandom", stream)
    proof = stark.prove(program, *matrices)
    assert stream.pos == g["urandom_bytes"]
    assert len(proof) == g["proof_len"] and hashlib.sha256(proof).hexdigest() == g["proof_sha256"]


def test_other_expansion_and_security_level():
    """log_expansion_factor 3, security_level 8, two grinding bits: (8 - 2) // 3 = 2 colinearity checks, folding by 4 over cosets; eight
    opened indices in a 2^12 domain"""
    m = mode(4, True, 2, log_expansion_factor=3, security_level=8)
    stark, proof = modes.prove_seeded("loop", m)
    assert (stark.fri.domain.length, stark.num_colinearity_checks, stark.expansion_factor) == (1 << 12, 2, 8)
    assert proof == modes.prove_seeded("loop", m, prepare=lambda s: setattr(s, "native_stages", False))[1]
    args = modes.stark_args(modes.PROGRAMS["loop"], m)
    for native in (True, False):
        assert outcome(args, proof, native) == ACCEPTED, "native" if native else "python"
    assert modes.make_stark(modes.PROGRAMS["loop"], m)._verify_native(proof) is True


def test_two_indices_in_one_coset_share_the_tuple_object():
    """DESIGN.md's identity rule, at a shape where it must apply: 34 indices into the 32 cosets of the 2^8 domain (and 17 colinearity
    checks on a last codeword of 32).  The same tuple object pushed twice is one pickle and a back-reference, so the drivers agree to
    the byte only if they agree on the rule"""
    S = 34
    m = mode(8, True, security_level=S)
    stark, proof = modes.prove_seeded("plus1", m)
    q = stark.fri.domain.length // 8
    assert len(stark._last["indices"]) == S and len({i % q for i in stark._last["indices"]}) <= q < S
    for prepare in (lambda s: setattr(s, "native_stages", False), lambda s: (setattr(s, "native_stages", False), setattr(s, "_openings_native", lambda p: None))):
        assert proof == modes.prove_seeded("plus1", m, prepare=prepare)[1]
    actual = pickle.loads(proof)
    rows = S * (1 + len(stark._layout.unit_distances(stark.fri.domain.length))) * 4
    opened = actual[8 + rows:8 + rows + 2 * S:2]
    first = {}
    for i, leaf in zip(stark._last["indices"], opened):
        assert isinstance(leaf, tuple) and len(leaf) == 8
        assert first.setdefault(i % q, leaf) is leaf, "one tuple object per coset"
    assert len({id(leaf) for leaf in opened}) == len(first)
    assert stark.verify(proof) is True
