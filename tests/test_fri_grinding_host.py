"""Proof-of-work grinding in FRI (Fri(..., grinding_bits=b)), host side, no GPU: the native predicate (bfs_pow_check) and the search
kernel's per-lane scan (csrc/pow_core.hpp through tests/emu/emu_pow.cpp) against hashlib, the nonce in the transcript against pickle,
the verifier against the streams of a CPython model (tests/fri_grinding_model.py), the rejections, the constructor's argument checks.
Every expectation is hashlib's, pickle's or the existing models'."""
import ctypes
import functools
import hashlib
import os
import pickle
import random
import sys

import pytest

from conftest import ROOT

import fri_coset_model
import fri_folding_model
import fri_grinding_model as model

SEED = 0x6B1D
OFFSET = 7
T = 4
BFS_ERR_BAD_ARG = 6
POW = "proof of work check failure\n"

# (N, expansion, a, coset leaves) with N = 2^5 .. 2^8, expansion 2 or 4 and at least one fold
SHAPES = [(N, e, a, coset) for N in (32, 64, 128, 256) for e in (2, 4) for a in (2, 4, 8) for coset in (False, True)
          if fri_folding_model.num_folds(N, e, a.bit_length() - 1) >= 1]
BITS = (1, 5, 9)
REJECT_SHAPES = [(64, 4, 2, False), (256, 4, 4, True), (128, 2, 8, True), (256, 2, 8, False)]


@pytest.fixture(scope="session")
def sb():
    from stark_brainfuck_amd import build
    build.build_library()
    import stark_brainfuck_amd
    return stark_brainfuck_amd


@pytest.fixture(scope="module")
def lib(sb):
    from stark_brainfuck_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def emu():
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    from build_emu import build_emulation
    e = ctypes.CDLL(build_emulation())
    u64 = ctypes.c_uint64
    e.emu_pow_search.argtypes = [ctypes.c_char_p, ctypes.c_uint, u64, u64, u64, ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_int)]
    e.emu_pow_hit.argtypes = [ctypes.c_char_p, u64, ctypes.c_uint]
    return e


def _seed(i):
    return hashlib.sha256(b"grinding seed %d" % i).digest()


@functools.lru_cache(maxsize=None)
def _model(N, expansion, a, coset, bits, codeword_seed=SEED, forced_nonce=None):
    """the model's proof -- computed once per case, shared, never changed"""
    from oracle import ref_oracle as o
    omega = o.primitive_nth_root(N)
    cw = fri_folding_model.codeword_of(o, codeword_seed + N + expansion, N, expansion, OFFSET, omega)
    out = model.prove(o, cw, OFFSET, omega, expansion, T, a, coset, bits, forced_nonce=forced_nonce)
    out["bytes"] = out["proof_stream"].serialize()
    out["codeword"] = cw
    return out


def _fri(sb, N, expansion, a, coset, bits):
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    assert BF.generator().value == OFFSET
    return sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, expansion, T, XF, folding_factor=a, coset_leaves=coset, grinding_bits=bits)


def _stream(sb, objects):
    ps = sb.ProofStream()
    ps.objects = list(objects)
    return ps


# ------------------------------------------------------------------------------------------------ 1. the predicate
def _check(lib, seed, bits, nonce):
    ok = ctypes.c_int(7)
    assert lib.bfs_pow_check(seed, bits, nonce, ctypes.byref(ok)) == 0
    assert ok.value in (0, 1)
    return bool(ok.value)


def test_pow_check_against_hashlib_on_random_triples(lib):
    rng = random.Random(SEED)
    seen = set()
    for i in range(200):
        seed, bits = _seed(i), rng.randint(1, 40)
        nonce = rng.choice([rng.getrandbits(64), rng.getrandbits(20), rng.getrandbits(33)])
        want = model.hit(seed, nonce, bits)
        assert _check(lib, seed, bits, nonce) is want, (i, bits, nonce)
        seen.add(want)
    assert seen == {False, True}


@pytest.mark.parametrize("bits", [1, 8, 12, 16])
def test_pow_check_on_the_smallest_nonce_and_the_one_before_it(lib, emu, bits):
    found = 0
    for i in range(4):
        seed = _seed(100 * bits + i)
        nonce = model.grind(seed, bits)
        assert _check(lib, seed, bits, nonce) is True and emu.emu_pow_hit(seed, nonce, bits) == 1
        if nonce:
            found += 1
            assert _check(lib, seed, bits, nonce - 1) is False and emu.emu_pow_hit(seed, nonce - 1, bits) == 0
        if bits < 40 and not model.hit(seed, nonce, bits + 1):
            assert _check(lib, seed, bits + 1, nonce) is False
    assert found or bits == 1


def test_pow_check_looks_at_the_first_eight_digest_bytes_little_endian(lib):
    """the word is digest[:8] little-endian, its TOP bits: a seed and nonce whose digest starts with a zero byte but whose eighth byte
    is not small is no 8-bit hit, and the other way round"""
    seed, kinds = _seed(1), set()
    for nonce in range(200000):
        d = hashlib.blake2b(seed + nonce.to_bytes(8, "little")).digest()
        if (d[0] == 0) != (d[7] == 0):
            assert _check(lib, seed, 8, nonce) is (d[7] == 0)
            kinds.add(d[7] == 0)
            if len(kinds) == 2:
                break
    assert len(kinds) == 2


def test_pow_check_bad_arguments(lib):
    ok = ctypes.c_int(7)
    for bits in (0, 41, 64, 1 << 31):
        assert lib.bfs_pow_check(_seed(0), bits, 0, ctypes.byref(ok)) == BFS_ERR_BAD_ARG
        assert b"bits" in lib.bfs_last_error() and ok.value == 7
    assert lib.bfs_pow_check(None, 8, 0, ctypes.byref(ok)) == BFS_ERR_BAD_ARG
    assert lib.bfs_pow_check(_seed(0), 8, 0, None) == BFS_ERR_BAD_ARG
    assert lib.bfs_pow_check(_seed(0), 40, (1 << 64) - 1, ctypes.byref(ok)) == 0 and ok.value == 0


def test_check_grinding_is_the_models_predicate(sb):
    from stark_brainfuck_amd.fri import check_grinding
    rng = random.Random(SEED + 1)
    for i in range(100):
        seed, bits, nonce = _seed(i), rng.randint(1, 12), rng.getrandbits(rng.choice([8, 64]))
        assert check_grinding(seed, nonce, bits) is model.hit(seed, nonce, bits)
    nonce = model.grind(_seed(5), 10)
    assert check_grinding(_seed(5), nonce, 10) is True and check_grinding(bytearray(_seed(5)), nonce, 10) is True


# ------------------------------------------------------------------------------------------------ 2. the nonce in the transcript
NONCES = [0, 255, 256, 65535, 65536, (1 << 31) - 1, 1 << 31, 1 << 32, 1 << 63, (1 << 64) - 1]


@pytest.mark.parametrize("nonce", NONCES)
def test_a_stream_that_holds_a_nonce_is_pickles_bytes(sb, lib, nonce):
    from stark_brainfuck_amd.ip import NativeTranscript
    objects = [hashlib.blake2b(b"root").digest(), [b"\x01" * 64], nonce, (hashlib.blake2b(b"x").digest(),)]
    want = pickle.dumps(objects)
    ps = _stream(sb, objects)
    assert ps.serialize() == want
    assert ps.prover_fiat_shamir() == hashlib.shake_256(want).digest(32)
    # natively, as bfs_fri_query pushes it
    t = NativeTranscript()
    t.push(objects[0]); t.push(objects[1])
    assert lib.bfs_ps_push(t.handle, lib.bfs_ps_obj_int(t.handle, nonce)) == 0
    t.push(objects[3])
    assert t.serialize() == want
    assert lib.bfs_ps_obj_kind(t.handle, lib.bfs_ps_object_at(t.handle, 2)) == 1
    assert t.to_python(lib.bfs_ps_object_at(t.handle, 2), None) == nonce
    # and back
    loaded = NativeTranscript.from_bytes(want)
    assert loaded is not None and loaded.num_objects() == 4 and loaded.serialize() == want
    back = loaded.to_python(lib.bfs_ps_object_at(loaded.handle, 2), None)
    assert type(back) is int and back == nonce
    vs = sb.ProofStream().deserialize(want)
    assert vs.objects == objects and type(vs.objects[2]) is int
    vs.read_index = 3
    assert vs.verifier_fiat_shamir() == hashlib.shake_256(pickle.dumps(objects[:3])).digest(32)


# ------------------------------------------------------------------------------------------------ 3. the kernel's scan, emulated
def _emu_search(emu, seed, bits, first, count, lanes):
    nonce, found = ctypes.c_uint64(123), ctypes.c_int(7)
    assert emu.emu_pow_search(seed, bits, first, count, lanes, ctypes.byref(nonce), ctypes.byref(found)) == 0
    return nonce.value if found.value else None


@pytest.mark.parametrize("lanes", [64, 256, 192])
@pytest.mark.parametrize("first", [0, (1 << 32) - 5, (1 << 63) + 3])
def test_scan_of_all_lanes_against_the_linear_search(emu, lanes, first):
    """bits = 5: windows of 1, 63, 64, 65 nonces mostly hold no hit or one, 1 000 hold about thirty"""
    outcomes = set()
    for i in range(6):
        seed = _seed(i)
        for count in (1, 63, 64, 65, 1000):
            want = model.grind(seed, 5, first, count)
            assert _emu_search(emu, seed, 5, first, count, lanes) == want, (i, count)
            hits = sum(model.hit(seed, first + j, 5) for j in range(count))
            outcomes.add(min(hits, 2))
    assert outcomes == {0, 1, 2}


@pytest.mark.parametrize("lanes", [64, 256, 192])
@pytest.mark.parametrize("first", [0, (1 << 32) - 5, (1 << 63) + 3])
def test_scan_of_windows_cut_at_the_hits(emu, lanes, first):
    """n1 < n2 the first two 9-bit hits from `first`: no hit, one hit on the first nonce, on the last nonce, on both ends, several"""
    seed = _seed(77)
    n1 = model.grind(seed, 9, first)
    n2 = model.grind(seed, 9, n1 + 1)
    search = lambda start, count: _emu_search(emu, seed, 9, start, count, lanes)
    if n1 > first:
        assert search(first, n1 - first) is None
    assert search(first, n1 - first + 1) == n1                 # the last nonce of the window
    assert search(n1, 1) == n1
    assert search(n1, n2 - n1) == n1                           # the first nonce, nothing behind it
    if n2 - n1 > 1:
        assert search(n1 + 1, n2 - n1 - 1) is None
    assert search(n1 + 1, n2 - n1) == n2
    assert search(n1, n2 - n1 + 1) == n1                       # both ends
    assert search(first, n2 - first + 1000) == n1              # several


def test_scan_up_to_the_last_nonce_there_is(emu):
    """a window that ends at 2^64 does not wrap; one beyond it is refused"""
    top = 1 << 64
    for i in range(3):
        seed = _seed(i)
        for count in (1, 64, 700):
            assert _emu_search(emu, seed, 4, top - count, count, 192) == model.grind(seed, 4, top - count, count)
    nonce, found = ctypes.c_uint64(), ctypes.c_int()
    assert emu.emu_pow_search(_seed(0), 4, top - 5, 6, 64, ctypes.byref(nonce), ctypes.byref(found)) == -1


# ------------------------------------------------------------------------------------------------ 4. the verifier against the model
def test_the_shapes_cover_what_they_should():
    assert {N for N, _, _, _ in SHAPES} == {32, 64, 128, 256} and {e for _, e, _, _ in SHAPES} == {2, 4}
    assert {(a, coset) for _, _, a, coset in SHAPES} == {(a, coset) for a in (2, 4, 8) for coset in (False, True)}
    assert all(shape in SHAPES for shape in REJECT_SHAPES)


@pytest.mark.parametrize("N,expansion,a,coset", SHAPES)
def test_without_grinding_the_model_is_the_existing_model(N, expansion, a, coset):
    from oracle import ref_oracle as o
    ref = _model(N, expansion, a, coset, 0)
    existing = (fri_coset_model if coset else fri_folding_model).prove(o, ref["codeword"], OFFSET, o.primitive_nth_root(N), expansion, T, a)
    assert ref["bytes"] == existing["proof_stream"].serialize() and ref["indices"] == existing["indices"]
    assert ref["nonce"] is None


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("N,expansion,a,coset", SHAPES)
def test_model_stream_is_accepted_and_consumed(sb, N, expansion, a, coset, bits, capsys):
    from oracle import ref_oracle as o
    ref, plain = _model(N, expansion, a, coset, bits), _model(N, expansion, a, coset, 0)
    F = ref["rounds"] - 1
    objects = ref["proof_stream"].objects
    # the commit phase is the mode's own; then the nonce, the smallest hit for the seed drawn over it
    assert len(objects) == len(plain["proof_stream"].objects) + 1
    assert o.dumps(objects[:F + 1]) == o.dumps(plain["proof_stream"].objects[:F + 1])
    assert type(objects[F + 1]) is int and objects[F + 1] == ref["nonce"]
    assert ref["seed"] == hashlib.shake_256(o.dumps(objects[:F + 1])).digest(32)
    assert model.hit(ref["seed"], ref["nonce"], bits) and not any(model.hit(ref["seed"], n, bits) for n in range(ref["nonce"]))
    fri = _fri(sb, N, expansion, a, coset, bits)
    assert fri.grinding_bits == bits
    capsys.readouterr()
    vs = sb.ProofStream().deserialize(ref["bytes"])
    assert fri.verify(vs, ref["roots"][0]) is True
    assert vs.read_index == len(vs.objects)
    assert fri.verify(_stream(sb, vs.objects), ref["roots"][0]) is True
    assert capsys.readouterr().out == ""


# ------------------------------------------------------------------------------------------------ 5. rejections
@pytest.mark.parametrize("N,expansion,a,coset", REJECT_SHAPES)
def test_a_wrong_or_missing_nonce_is_rejected_without_raising(sb, N, expansion, a, coset, capsys):
    bits = 5
    ref = _model(N, expansion, a, coset, bits)
    fri = _fri(sb, N, expansion, a, coset, bits)
    root0, at = ref["roots"][0], ref["rounds"]                 # F roots and the last codeword in front of the nonce
    objects = sb.ProofStream().deserialize(ref["bytes"]).objects
    assert objects[at] == ref["nonce"]

    def verdict(objs, verifier=fri, root=root0):
        capsys.readouterr()
        return verifier.verify(_stream(sb, objs), root), capsys.readouterr().out

    assert verdict(objects) == (True, "")
    # the nonce plus one: no hit, or (one time in 32) a hit that samples other indices
    ok, said = verdict(objects[:at] + [ref["nonce"] + 1] + objects[at + 1:])
    assert ok is False and (said == POW or model.hit(ref["seed"], ref["nonce"] + 1, bits))
    # a nonce that is no hit, in a stream that is the honest prover's in everything else: the queries answer the indices drawn over it
    miss = next(n for n in range(1 << 20) if not model.hit(ref["seed"], n, bits))
    forged = _model(N, expansion, a, coset, bits, forced_nonce=miss)
    assert forged["nonce"] == miss and forged["seed"] == ref["seed"] and forged["roots"] == ref["roots"]
    assert verdict(sb.ProofStream().deserialize(forged["bytes"]).objects) == (False, POW)
    # (and with a nonce that does hit, forced the same way, it is accepted: the proof of work is all that stream lacks)
    second = model.grind(ref["seed"], bits, ref["nonce"] + 1)
    assert verdict(sb.ProofStream().deserialize(_model(N, expansion, a, coset, bits, forced_nonce=second)["bytes"]).objects) == (True, "")
    # things that are no nonce
    for bad in (True, False, -1, 1 << 64, b"\x00", (ref["nonce"],), [ref["nonce"]], None, float(ref["nonce"])):
        assert verdict(objects[:at] + [bad] + objects[at + 1:]) == (False, POW), repr(bad)
    # no nonce at all: a stream made without grinding, and the grinding stream with its nonce cut out
    plain = _model(N, expansion, a, coset, 0)
    assert verdict(sb.ProofStream().deserialize(plain["bytes"]).objects) == (False, POW)
    assert verdict(objects[:at] + objects[at + 1:]) == (False, POW)
    # and a verifier that expects no nonce does not take the grinding stream
    assert _fri(sb, N, expansion, a, coset, 0).verify(sb.ProofStream().deserialize(plain["bytes"]), root0) is True
    if a == 2 and not coset:
        with pytest.raises(TypeError):          # (the reference's verifier: it unpacks what it pulls without looking)
            _fri(sb, N, expansion, a, coset, 0).verify(sb.ProofStream().deserialize(ref["bytes"]), root0)
    else:
        assert _fri(sb, N, expansion, a, coset, 0).verify(sb.ProofStream().deserialize(ref["bytes"]), root0) is False


@pytest.mark.parametrize("N,expansion,a,coset", REJECT_SHAPES[:2])
def test_a_proof_ground_to_fewer_bits_than_the_verifier_asks_for(sb, N, expansion, a, coset, capsys):
    """a 5-bit proof whose nonce is no 6-bit hit (the codeword is searched for on the CPU so that it is not) under a 6-bit verifier"""
    for codeword_seed in range(SEED, SEED + 64):
        ref = _model(N, expansion, a, coset, 5, codeword_seed=codeword_seed)
        if not model.hit(ref["seed"], ref["nonce"], 6):
            break
    else:
        pytest.fail("no codeword whose 5-bit nonce misses 6 bits among 64")
    assert _fri(sb, N, expansion, a, coset, 5).verify(sb.ProofStream().deserialize(ref["bytes"]), ref["roots"][0]) is True
    capsys.readouterr()
    assert _fri(sb, N, expansion, a, coset, 6).verify(sb.ProofStream().deserialize(ref["bytes"]), ref["roots"][0]) is False
    assert capsys.readouterr().out == POW


# ------------------------------------------------------------------------------------------------ 6. the constructor
def test_constructor_argument_checks(sb):
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    make = lambda **kw: sb.Fri(BF.generator(), BF.primitive_nth_root(1024), 1024, 4, T, XF, **kw)
    assert make().grinding_bits == 0 and make(folding_factor=8, coset_leaves=True).grinding_bits == 0
    for bits in (0, 1, 16, 40):
        for kw in ({}, {"folding_factor": 4}, {"folding_factor": 8, "coset_leaves": True}):
            fri = make(grinding_bits=bits, **kw)
            assert fri.grinding_bits == bits and fri._grinding_window is None
            assert fri.num_rounds() == make(**kw).num_rounds()
    for bad in (True, False, -1, 41, 64, 8.0, "8", None, (8,)):
        with pytest.raises(AssertionError, match="grinding_bits"):
            make(grinding_bits=bad)
