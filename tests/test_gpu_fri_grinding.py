"""Proof-of-work grinding on the GPU (bfs_pow_search, bfs_fri_session_set_grinding, Fri(..., grinding_bits=b), fri.grind): the nonce
search against hashlib's linear search, Fri.prove byte for byte against a CPython model of the protocol (tests/fri_grinding_model.py).
Integer hashing throughout: no tolerance anywhere.

No painted-arena case: the search reads and writes no device memory of the caller's.  Its arguments are a seed, two counters and a bit
count passed by value, and the eight bytes its lanes write are the library's own allocation."""
import ctypes
import functools
import hashlib
import os
import subprocess
import sys

import pytest

from conftest import ROOT

import fri_folding_model as per_element
import fri_grinding_model as model

pytestmark = pytest.mark.gpu

SEED = 0x6B1D
OFFSET = 7
EXPANSION = 4
T = 2
BFS_ERR_BAD_ARG = 6
u64 = ctypes.c_uint64
# a launch of the search takes 2^(bits + 2) nonces, at least LAUNCH_MIN (one workgroup of 256 threads, 16 nonces each)
LAUNCH_MIN = 4096


@pytest.fixture(scope="module")
def sb():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import stark_brainfuck_amd
    from stark_brainfuck_amd import _lib
    _lib.load()            # raises BackendUnavailable if the HIP library is missing: no fallback
    return stark_brainfuck_amd


@pytest.fixture(scope="module")
def lib(sb):
    from stark_brainfuck_amd import _lib
    return _lib.load()


def _seed(i):
    return hashlib.sha256(b"grinding seed %d" % i).digest()


def _search(lib, seed, bits, first, count, stream=0):
    nonce, found = u64(0xABCD), ctypes.c_int(7)
    rc = lib.bfs_pow_search(seed, bits, first, count, ctypes.byref(nonce), ctypes.byref(found), stream)
    assert rc == 0, lib.bfs_last_error()
    assert found.value in (0, 1)
    return nonce.value if found.value else None


@functools.lru_cache(maxsize=None)
def _first_hit(i, bits, first=0):
    return model.grind(_seed(i), bits, first)


# ------------------------------------------------------------------------------------------------ 1. the search
@pytest.mark.parametrize("bits", [1, 8, 16])
def test_search_against_hashlib(sb, lib, bits):
    from stark_brainfuck_amd.fri import grind
    for i in range(4 if bits < 16 else 2):
        want = _first_hit(i, bits)
        assert grind(_seed(i), bits) == want                               # up to 2^(bits + 6) nonces
        assert _search(lib, _seed(i), bits, 0, want + 1) == want
        assert grind(_seed(i), bits, first_nonce=want + 1, count=1 << (bits + 6)) == _first_hit(i, bits, want + 1)


def test_search_of_twenty_bits(lib):
    """740 972 hashlib calls for the expectation; the search is one launch of 2^22 nonces"""
    want = _first_hit(3, 20)
    assert _search(lib, _seed(3), 20, 0, 1 << 26) == want
    if want:
        assert _search(lib, _seed(3), 20, 0, want) is None


def test_windows_cut_at_the_first_two_hits(lib):
    seed = _seed(12)
    n1 = _first_hit(12, 12)
    n2 = _first_hit(12, 12, n1 + 1)
    assert 0 < n1 and n1 + 1 < n2
    search = lambda first, count: _search(lib, seed, 12, first, count)
    assert search(0, n1) is None
    assert search(0, n1 + 1) == n1
    assert search(n1, 1) == n1
    assert search(n1 + 1, n2 - n1 - 1) is None
    assert search(n1 + 1, n2 - n1) == n2
    assert search(0, n2 + 1) == n1


@pytest.mark.parametrize("count", [1, 63, 64, 65, 1000003])
def test_window_sizes(lib, count):
    """5 bits: the small windows hold no hit, one or a few; 1 000 003 nonces are 245 launches' worth, of which the first with a hit ends
    the search; at 24 bits they are one launch that scans them all"""
    outcomes = set()
    for i in range(8):
        for first in (0, 1000 * i + 7):
            want = model.grind(_seed(i), 5, first, count)
            assert _search(lib, _seed(i), 5, first, count) == want, (i, first)
            outcomes.add(want is None)
    assert outcomes == ({False, True} if count <= 65 else {False})
    if count == 1000003:
        assert _search(lib, _seed(0), 24, 0, count) == model.grind(_seed(0), 24, 0, count)


def test_a_search_that_goes_through_several_launches_without_a_hit(lib):
    """10 bits: launches of LAUNCH_MIN nonces; a seed (found with hashlib) whose first hit lies behind the first launch"""
    i = next(i for i in range(2000) if model.grind(_seed(i), 10, 0, LAUNCH_MIN) is None)
    want = _first_hit(i, 10)
    assert want >= LAUNCH_MIN
    assert _search(lib, _seed(i), 10, 0, 1 << 16) == want
    assert _search(lib, _seed(i), 10, 0, want) is None
    assert _search(lib, _seed(i), 10, 5, want - 5 + 1) == want


@pytest.mark.parametrize("first", [(1 << 32) - 5, (1 << 63) + 3])
@pytest.mark.parametrize("bits", [8, 16])
def test_search_from_a_large_first_nonce(lib, first, bits):
    """a nonce cut to 32 bits, or a window start added in 32 bits, finds another hit"""
    for i in range(2):
        want = _first_hit(i, bits, first)
        assert want >= first
        assert _search(lib, _seed(i), bits, first, 1 << (bits + 6)) == want
        assert _search(lib, _seed(i), bits, first, want - first + 1) == want
        if want > first:
            assert _search(lib, _seed(i), bits, first, want - first) is None


def test_a_window_that_ends_at_two_to_the_64(lib):
    top = 1 << 64
    for i in range(3):
        for count in (1, 5, 5000):
            assert _search(lib, _seed(i), 3, top - count, count) == model.grind(_seed(i), 3, top - count, count)


def test_two_streams_one_after_the_other(lib):
    from stark_brainfuck_amd import _lib
    streams = [ctypes.c_void_p(), ctypes.c_void_p()]
    for s in streams:
        _lib.check(lib.bfs_stream_create(ctypes.byref(s)))
    try:
        for i, s in enumerate(streams + streams):
            assert _search(lib, _seed(20 + i), 12, 0, 1 << 18, stream=s) == _first_hit(20 + i, 12)
        assert _search(lib, _seed(20), 12, 0, 1 << 18) == _first_hit(20, 12)
    finally:
        for s in streams:
            _lib.check(lib.bfs_stream_destroy(s))


def test_search_bad_arguments(lib):
    nonce, found = u64(0xABCD), ctypes.c_int(7)
    call = lambda seed, bits, first, count: lib.bfs_pow_search(seed, bits, first, count, ctypes.byref(nonce), ctypes.byref(found), 0)
    for bits in (0, 41, 64):
        assert call(_seed(0), bits, 0, 100) == BFS_ERR_BAD_ARG and b"bits" in lib.bfs_last_error()
    assert call(_seed(0), 8, 0, 0) == BFS_ERR_BAD_ARG and b"empty" in lib.bfs_last_error()
    assert call(_seed(0), 8, (1 << 64) - 5, 6) == BFS_ERR_BAD_ARG and b"wraps" in lib.bfs_last_error()
    assert call(_seed(0), 8, 1, (1 << 64) - 1) == 0 and found.value == 1 and nonce.value == _first_hit(0, 8, 1)
    nonce.value, found.value = 0xABCD, 7
    assert call(_seed(0), 8, 2, (1 << 64) - 1) == BFS_ERR_BAD_ARG
    assert call(None, 8, 0, 100) == BFS_ERR_BAD_ARG
    assert lib.bfs_pow_search(_seed(0), 8, 0, 100, None, ctypes.byref(found), 0) == BFS_ERR_BAD_ARG
    assert lib.bfs_pow_search(_seed(0), 8, 0, 100, ctypes.byref(nonce), None, 0) == BFS_ERR_BAD_ARG
    assert (nonce.value, found.value) == (0xABCD, 7)                       # a refused call writes nothing


# ------------------------------------------------------------------------------------------------ 2. Fri.prove against the model
def _prepushed(make_element, oracle):
    """objects in front of the proof -- a digest, a tuple of elements, a list of digests -- with enough digests (6.4 KB) that the native
    prover's Fiat-Shamir look-ahead takes them as its prefix"""
    digests = [hashlib.blake2b(bytes([i])).digest() for i in range(101)]
    elements = [make_element([oracle.felt(SEED + 88, 3 * i + j) for j in range(3)]) for i in range(3)]
    return [digests[0], tuple(elements), digests[1:]]


@functools.lru_cache(maxsize=None)
def _reference(a, N, coset, bits, prepushed=False):
    """the model's proof of the seeded codeword -- computed once per case, shared, never changed"""
    from oracle import ref_oracle as o
    omega = o.primitive_nth_root(N)
    cw = per_element.codeword_of(o, SEED + N + EXPANSION, N, EXPANSION, OFFSET, omega)
    ps = None
    if prepushed:
        ps = o.ProofStreamOracle()
        for obj in _prepushed(o.make_xfe, o):
            ps.push(obj)
    out = model.prove(o, cw, OFFSET, omega, EXPANSION, T, a, coset, bits, proof_stream=ps)
    out["bytes"] = out["proof_stream"].serialize()
    out["codeword"] = cw
    return out


def _fri(sb, a, N, coset, bits=None, XF=None):
    XF = sb.ExtensionField.main() if XF is None else XF
    BF = XF.modulus.coefficients[0].field
    assert BF.generator().value == OFFSET
    kw = {} if bits is None else {"grinding_bits": bits}
    return sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, EXPANSION, T, XF, folding_factor=a, coset_leaves=coset, **kw)


# (a, N, coset leaves, bits): every folding factor in both modes with every bit count, N = 2^6 .. 2^12 and one 2^17
PROVE_CASES = [(2, 1 << 6, False, 1), (2, 1 << 7, True, 8), (2, 1 << 9, False, 12), (2, 1 << 12, True, 1), (2, 1 << 10, False, 8), (2, 1 << 8, True, 12),
               (4, 1 << 6, True, 8), (4, 1 << 8, False, 12), (4, 1 << 10, True, 1), (4, 1 << 11, False, 8), (4, 1 << 12, True, 12), (4, 1 << 9, False, 1),
               (8, 1 << 6, False, 12), (8, 1 << 9, True, 1), (8, 1 << 12, False, 8), (8, 1 << 10, True, 12), (8, 1 << 11, False, 1), (8, 1 << 17, True, 8)]


def test_prove_cases_cover_every_mode_with_every_bit_count():
    assert {(a, coset) for a, _, coset, _ in PROVE_CASES} == {(a, coset) for a in (2, 4, 8) for coset in (False, True)}
    assert {(a, bits) for a, _, _, bits in PROVE_CASES} == {(a, bits) for a in (2, 4, 8) for bits in (1, 8, 12)}
    assert {(coset, bits) for _, _, coset, bits in PROVE_CASES} == {(coset, bits) for coset in (False, True) for bits in (1, 8, 12)}
    assert {N for _, N, _, _ in PROVE_CASES} == {1 << e for e in range(6, 13)} | {1 << 17}


def _check_proof(sb, fri, ref, ps, top, read_from=0):
    assert top == ref["indices"]
    assert len(ps.objects) == len(ref["proof_stream"].objects)
    assert ps.serialize() == ref["bytes"]
    at = read_from + ref["rounds"]
    assert type(ps.objects[at]) is int and ps.objects[at] == ref["nonce"]
    vs = sb.ProofStream()
    vs.objects, vs.read_index = list(ps.objects), read_from
    assert fri.verify(vs, ref["roots"][0]) is True and vs.read_index == len(vs.objects)
    if not read_from:
        assert fri.verify(sb.ProofStream().deserialize(ps.serialize()), ref["roots"][0]) is True


@pytest.mark.parametrize("a,N,coset,bits", PROVE_CASES)
def test_prove_is_the_model_byte_for_byte(sb, a, N, coset, bits):
    ref = _reference(a, N, coset, bits)
    assert model.hit(ref["seed"], ref["nonce"], bits)
    fri = _fri(sb, a, N, coset, bits)
    assert fri.num_rounds() == ref["rounds"]
    ps = sb.ProofStream()
    top = fri.prove(sb.XArray.from_numpy(ref["codeword"]), ps)
    _check_proof(sb, fri, ref, ps, top)
    if bits == 12:
        bad = sb.ProofStream()
        bad.objects = list(ps.objects)
        bad.objects[ref["rounds"]] += 1
        assert fri.verify(bad, ref["roots"][0]) is False


@pytest.mark.parametrize("a,N,coset", [(2, 1 << 9, False), (4, 1 << 12, True), (8, 1 << 10, True)])
@pytest.mark.parametrize("window", [64, 1 << 20])
def test_prove_with_a_search_window_of_the_callers(sb, a, N, coset, window):
    """windows of 64 nonces: the search crosses dozens of them before the one with the hit (12 bits: the nonce is around 4 096); a
    window larger than the answer: one step"""
    ref = _reference(a, N, coset, 12)
    assert ref["nonce"] >= 10 * 64 if window == 64 else window > ref["nonce"]
    fri = _fri(sb, a, N, coset, 12)
    fri._grinding_window = window
    ps = sb.ProofStream()
    top = fri.prove(sb.XArray.from_numpy(ref["codeword"]), ps)
    _check_proof(sb, fri, ref, ps, top)


@pytest.mark.parametrize("a,N,coset", [(2, 1 << 10, False), (4, 1 << 12, True), (8, 1 << 10, False)])
def test_prove_behind_objects_pushed_beforehand(sb, oracle, a, N, coset):
    ref = _reference(a, N, coset, 8, prepushed=True)
    XF = sb.ExtensionField.main()
    ps = sb.ProofStream()
    pre = _prepushed(XF.from_limbs, oracle)
    for obj in pre:
        ps.push(obj)
    fri = _fri(sb, a, N, coset, 8, XF=XF)
    top = fri.prove(sb.XArray.from_numpy(ref["codeword"]), ps)
    _check_proof(sb, fri, ref, ps, top, read_from=len(pre))


_CHILD = r"""
import hashlib, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import stark_brainfuck_amd as sb
import test_gpu_fri_grinding as T
from oracle import ref_oracle as o
XF = sb.ExtensionField.main()
for a, N, coset in T.LOOKAHEAD_CASES:
    cw = T.per_element.codeword_of(o, T.SEED + N + T.EXPANSION, N, T.EXPANSION, T.OFFSET, o.primitive_nth_root(N))
    for pre in (False, True):
        ps = sb.ProofStream()
        if pre:
            for obj in T._prepushed(XF.from_limbs, o):
                ps.push(obj)
        top = T._fri(sb, a, N, coset, 8, XF).prove(sb.XArray.from_numpy(cw), ps)
        print("RESULT", a, coset, pre, top, hashlib.sha256(ps.serialize()).hexdigest())
"""
LOOKAHEAD_CASES = [(2, 1 << 10, False), (8, 1 << 10, True)]


def test_prove_without_the_lookahead(sb):
    """the look-ahead switch is read once per process: BFS_FRI_LOOKAHEAD=0 gets a process of its own"""
    want = []
    for a, N, coset in LOOKAHEAD_CASES:
        for pre in (False, True):
            ref = _reference(a, N, coset, 8, prepushed=pre)
            want.append("RESULT %s %s %s %s %s" % (a, coset, pre, ref["indices"], hashlib.sha256(ref["bytes"]).hexdigest()))
    env = dict(os.environ)
    env["BFS_FRI_LOOKAHEAD"] = "0"
    res = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:]
    assert [line for line in res.stdout.splitlines() if line.startswith("RESULT")] == want


@pytest.mark.parametrize("a,N,coset", [(2, 1 << 10, False), (4, 1 << 12, True), (8, 1 << 10, True)])
def test_a_proof_with_the_callers_round0_tree_is_the_same_proof(sb, a, N, coset):
    ref = _reference(a, N, coset, 8)
    fri = _fri(sb, a, N, coset, 8)
    cw = sb.XArray.from_numpy(ref["codeword"])
    tree = sb.CosetMerkle(cw, a) if coset else sb.Merkle(cw)
    assert tree.root() == ref["roots"][0]
    ps = sb.ProofStream()
    top = fri.prove(cw, ps, round0_tree=tree)
    _check_proof(sb, fri, ref, ps, top)


@pytest.mark.parametrize("a,N,coset", [(4, 1 << 10, True), (2, 1 << 9, False)])
def test_commit_pushes_no_nonce_and_the_python_mirror_grinds_itself(sb, a, N, coset):
    """grinding belongs to prove: Fri.commit alone leaves the stream at the last codeword.  The caller's own query phase -- fri.grind,
    push, sample, query / query_last -- writes what prove writes."""
    from stark_brainfuck_amd.fri import check_grinding, grind
    bits = 12
    ref = _reference(a, N, coset, bits)
    fri = _fri(sb, a, N, coset, bits)
    ps = sb.ProofStream()
    codewords, trees = fri.commit(sb.XArray.from_numpy(ref["codeword"]), ps)
    F = ref["rounds"] - 1
    assert len(ps.objects) == F + 1 and isinstance(ps.objects[-1], list)          # F roots and the last codeword: no nonce
    seed = ps.prover_fiat_shamir()
    assert seed == ref["seed"]
    nonce = grind(seed, bits)
    assert nonce == ref["nonce"] and check_grinding(seed, nonce, bits)
    ps.push(nonce)
    top = fri.sample_indices(ps.prover_fiat_shamir(), len(codewords[1]), len(codewords[-1]), T)
    assert top == ref["indices"]
    for i in range(F - 1):
        fri.query(trees[i], trees[i + 1], [x % len(codewords[i + 1]) for x in top], ps)
    fri.query_last(trees[-1], codewords[-1], [x % len(codewords[-1]) for x in top], ps)
    assert ps.serialize() == ref["bytes"]


# ------------------------------------------------------------------------------------------------ 3. the default is untouched
@pytest.mark.parametrize("a,N", [(2, 1 << 10), (4, 1 << 10)])
def test_the_default_after_a_grinding_proof_is_the_per_element_model(sb, oracle, a, N):
    ref = _reference(a, N, False, 8)
    cw = sb.XArray.from_numpy(ref["codeword"])
    ps = sb.ProofStream()
    fri = _fri(sb, a, N, False, 8)
    _check_proof(sb, fri, ref, ps, fri.prove(cw, ps))
    old = per_element.prove(oracle, ref["codeword"], OFFSET, oracle.primitive_nth_root(N), EXPANSION, T, a)
    if a == 2:
        theirs = oracle.fri_prove(ref["codeword"], OFFSET, oracle.primitive_nth_root(N), EXPANSION, T)
        assert theirs["proof_stream"].serialize() == old["proof_stream"].serialize()
    for bits in (None, 0):
        plain = _fri(sb, a, N, False, bits)
        assert plain.grinding_bits == 0
        ps = sb.ProofStream()
        assert plain.prove(cw, ps) == old["indices"]
        assert ps.serialize() == old["proof_stream"].serialize()
        assert plain.verify(sb.ProofStream().deserialize(ps.serialize()), old["roots"][0]) is True
    ps = sb.ProofStream()
    _check_proof(sb, fri, ref, ps, fri.prove(cw, ps))


# ------------------------------------------------------------------------------------------------ 4. the session switch
def test_session_argument_checks(sb, lib, oracle):
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.ip import NativeTranscript
    N = 256
    omega = oracle.primitive_nth_root(N)
    host = per_element.codeword_of(oracle, SEED + N + EXPANSION, N, EXPANSION, OFFSET, omega)
    cw = sb.XArray.from_numpy(host)
    session = lib.bfs_fri_session_new()
    try:
        for bits in (41, 64, 1 << 31):
            assert lib.bfs_fri_session_set_grinding(session, bits, 0) == BFS_ERR_BAD_ARG and b"bits" in lib.bfs_last_error()
        assert lib.bfs_fri_session_set_grinding(session, 40, 0) == 0
        assert lib.bfs_fri_session_set_grinding(session, 0, 5) == 0
        assert lib.bfs_fri_session_set_grinding(session, 8, 100) == 0
        transcript = NativeTranscript()
        _lib.check(lib.bfs_fri_commit(session, transcript.handle, cw.ptr, cw.stride, 8, OFFSET, omega, EXPANSION, 0))
        for bits in (0, 8):
            assert lib.bfs_fri_session_set_grinding(session, bits, 0) == BFS_ERR_BAD_ARG and b"already committed" in lib.bfs_last_error()
        top = (u64 * T)()
        _lib.check(lib.bfs_fri_query(session, transcript.handle, T, top, 0))
        ref = _reference(2, N, False, 8)                 # the session kept the 8 bits it was given before the commit, with windows of 100
        assert list(top) == ref["indices"] and transcript.serialize() == ref["bytes"]
    finally:
        lib.bfs_fri_session_free(session)
    # the one-shot entries do not grind
    transcript = NativeTranscript()
    top = (u64 * T)()
    _lib.check(lib.bfs_fri_prove(transcript.handle, cw.ptr, cw.stride, 8, OFFSET, omega, EXPANSION, T, top, 0))
    plain = _reference(2, N, False, 0)
    assert plain["nonce"] is None and list(top) == plain["indices"] and transcript.serialize() == plain["bytes"]
