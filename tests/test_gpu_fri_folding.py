"""FRI folding by 4 or 8 per round on the GPU (Fri(..., folding_factor=a), bfs_xfe_fold_multi, bfs_fri_session_set_folding), bit
for bit against a CPython model of the protocol (tests/fri_folding_model.py) whose every fold is the reference's fri.py:127-128
through oracle.fri_fold.  Integer arithmetic and byte hashing throughout: no tolerance anywhere."""
import ctypes
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import fri_folding_model as model

pytestmark = pytest.mark.gpu

SEED = 0xF01D
OFFSET = 7
P = (1 << 64) - (1 << 32) + 1
BFS_ERR_BAD_ARG = 6


@pytest.fixture(scope="module")
def sb():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import stark_brainfuck_amd
    from stark_brainfuck_amd import _lib
    _lib.load()            # raises BackendUnavailable if the HIP library is missing: no fallback
    return stark_brainfuck_amd


def _fri(sb, N, expansion, t, a=None, XF=None):
    """XF: the field object of elements already in the stream -- pickle writes a second field object out in full, the reference has one"""
    XF = sb.ExtensionField.main() if XF is None else XF
    BF = XF.modulus.coefficients[0].field
    assert BF.generator().value == OFFSET
    if a is None:
        return sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, expansion, t, XF)
    return sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, expansion, t, XF, folding_factor=a)


# ------------------------------------------------------------------------------------------------ 1. the fold on its own
def _fold_input(oracle, log_n, stride, seed):
    """(3, stride) words: a codeword of 2^log_n elements with 0 and p - 1 among its limbs, and junk behind it when stride > n"""
    n = 1 << log_n
    soa = oracle.felt_array(seed, 0, 3 * stride).reshape(3, stride).copy()
    soa[0, 0], soa[1, 0], soa[2, n - 1], soa[0, n // 2] = 0, P - 1, P - 1, 0
    if n >= 8:
        soa[:, 5] = 0
        soa[:, n - 3] = P - 1
    return soa


def _fold_multi(sb, soa, log_n, k, alpha, omega, out_stride):
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer, synchronize
    src = DeviceBuffer.from_numpy(np.ascontiguousarray(soa).reshape(-1))
    guard = np.full(3 * out_stride, 0xDEADBEEF, dtype=np.uint64)
    dst = DeviceBuffer.from_numpy(guard)
    _lib.check(_lib.load().bfs_xfe_fold_multi(src.ptr, soa.shape[1], dst.ptr, out_stride, log_n, k, (ctypes.c_uint64 * 3)(*alpha), OFFSET, omega, 0))
    synchronize(0)
    return dst.to_numpy().reshape(3, out_stride)


def _oracle_fold_k(oracle, cw, alpha, omega, k):
    return model.fold_round(oracle, cw, alpha, OFFSET, omega, k)[0]


@pytest.mark.parametrize("k", [2, 3])
def test_fold_multi_against_the_oracle(sb, oracle, k):
    for log_n in sorted({k, k + 1, 6, 11, 14}):
        n = 1 << log_n
        soa = _fold_input(oracle, log_n, n, SEED + 16 * k + log_n)
        alpha = [int(x) for x in oracle.felt_array(SEED + 99, 3 * log_n, 3)]
        omega = oracle.primitive_nth_root(n)
        got = _fold_multi(sb, soa, log_n, k, alpha, omega, n >> k)
        want = _oracle_fold_k(oracle, soa, alpha, omega, k)
        assert want.shape == (3, n >> k) and np.array_equal(got, want), "log_n = %d" % log_n


@pytest.mark.parametrize("k", [2, 3])
def test_fold_multi_with_strides_longer_than_the_codewords(sb, oracle, k):
    log_n = 9
    n, in_stride, out_stride = 1 << log_n, (1 << log_n) + 37, ((1 << log_n) >> k) + 11
    soa = _fold_input(oracle, log_n, in_stride, SEED + 7 * k)
    alpha = [P - 1, 0, 12345]
    omega = oracle.primitive_nth_root(n)
    got = _fold_multi(sb, soa, log_n, k, alpha, omega, out_stride)
    assert np.array_equal(got[:, :n >> k], _oracle_fold_k(oracle, soa[:, :n], alpha, omega, k))
    assert (got[:, n >> k:] == 0xDEADBEEF).all(), "words behind the folded codeword were written"


@pytest.mark.parametrize("k", [2, 3])
def test_fold_multi_beyond_one_pass_of_the_grid(sb, oracle, k):
    """the fold kernel's grid is capped at 4096 workgroups of 256 threads = 2^20 outputs; 2^21 outputs send every thread round its
    loop twice.  Checked against bfs_xfe_fold applied k times on the GPU (itself checked against the oracle in test_gpu_parity)."""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer, synchronize
    log_n = 21 + k
    n = 1 << log_n
    soa = _fold_input(oracle, log_n, n, SEED + 1000 + k)
    alpha = [int(x) for x in oracle.felt_array(SEED + 5, 0, 3)]
    omega = oracle.primitive_nth_root(n)
    lib = _lib.load()
    src = DeviceBuffer.from_numpy(soa.reshape(-1))
    multi = DeviceBuffer(3 * (n >> k))
    _lib.check(lib.bfs_xfe_fold_multi(src.ptr, n, multi.ptr, n >> k, log_n, k, (ctypes.c_uint64 * 3)(*alpha), OFFSET, omega, 0))
    cur, a, g, w, length = src, list(alpha), OFFSET, omega, n
    for step in range(k):
        nxt = DeviceBuffer(3 * (length // 2))
        _lib.check(lib.bfs_xfe_fold(cur.ptr, length, nxt.ptr, length // 2, log_n - step, (ctypes.c_uint64 * 3)(*a), g, w, 0))
        cur, length = nxt, length // 2
        a, g, w = model._xsquare_from_mul(oracle, a), oracle.mul(g, g), oracle.mul(w, w)
    synchronize(0)
    got, want = multi.to_numpy(), cur.to_numpy()
    assert length == n >> k and np.array_equal(got, want)
    assert (got < np.uint64(P)).all()


# ------------------------------------------------------------------------------------------------ 2. Fri.prove against the model
@functools.lru_cache(maxsize=None)
def _reference(N, expansion, t, a, prepushed=False):
    """the model's proof of the seeded codeword -- computed once per case, shared, never changed"""
    from oracle import ref_oracle as o
    omega = o.primitive_nth_root(N)
    cw = model.codeword_of(o, SEED + N + expansion, N, expansion, OFFSET, omega)
    ps = o.ProofStreamOracle()
    if prepushed:
        for obj in _prepushed(lambda limbs: o.make_xfe(limbs), o):
            ps.push(obj)
    out = model.prove(o, cw, OFFSET, omega, expansion, t, a, proof_stream=ps)
    out["bytes"] = ps.serialize()
    out["codeword"] = cw
    return out


def _prepushed(make_element, oracle):
    """objects in front of the proof, as in the golden case d16_t2_prepushed -- a digest, a tuple of elements, a list of digests --
    with enough digests (6.4 KB) that the native prover's Fiat-Shamir look-ahead takes them as its prefix"""
    digests = [hashlib.blake2b(bytes([i])).digest() for i in range(101)]
    elements = [make_element([oracle.felt(SEED + 88, 3 * i + j) for j in range(3)]) for i in range(3)]
    return [digests[0], tuple(elements), digests[1:]]


PROVE_CASES = [(4, 1 << 5, 4, 4), (4, 1 << 10, 4, 4), (4, 1 << 13, 4, 4), (4, 1 << 16, 4, 4), (4, 1 << 17, 4, 4),
               (8, 1 << 6, 4, 4), (8, 1 << 11, 4, 4), (8, 1 << 16, 4, 4),
               (4, 1 << 10, 16, 8)]


def test_prove_cases_put_a_round_on_every_fold_site():
    """rounds >= 1 are produced by a fold: above 16384 elements inside the leaf kernel, at 16384 and at 8192 by the two tree paths of
    the one-launch round kernel, below that by the same kernel with a single launch for the whole tree (64 and fewer: one workgroup)"""
    produced = {(a, N >> (k * r)) for a, N, e, _ in PROVE_CASES for k in [a.bit_length() - 1]
                for r in range(1, model.num_folds(N, e, k) + 1)}
    for a in (4, 8):
        sizes = {n for a_, n in produced if a_ == a}
        assert 16384 in sizes or a == 8, sizes
        assert 8192 in sizes and any(64 < n < 8192 for n in sizes) and any(n <= 64 for n in sizes), sizes
    assert (4, 1 << 15) in produced            # (a = 8 above 16384: test_commit_by_eight_at_2p18_and_2p19)


@pytest.mark.parametrize("a,N,expansion,t", PROVE_CASES)
def test_prove_is_the_model_byte_for_byte(sb, a, N, expansion, t):
    ref = _reference(N, expansion, t, a)
    fri = _fri(sb, N, expansion, t, a)
    assert fri.num_rounds() == ref["rounds"]
    cw = sb.XArray.from_numpy(ref["codeword"])
    ps = sb.ProofStream()
    assert fri.prove(cw, ps) == ref["indices"]
    assert len(ps.objects) == len(ref["proof_stream"].objects)
    assert ps.serialize() == ref["bytes"]
    vs = sb.ProofStream()
    vs.objects = list(ps.objects)
    assert fri.verify(vs, ref["roots"][0]) is True
    assert vs.read_index == len(vs.objects)
    if (a, N) in ((4, 1 << 10), (8, 1 << 11)):
        bad = sb.ProofStream()
        bad.objects = list(ps.objects)
        bad.objects[0] = bytes(64)           # a wrong round-1 root changes every later challenge
        assert fri.verify(bad, ref["roots"][0]) is False


# ------------------------------------------------------------------------------------------------ 3. commit, folding by 8, large
@pytest.mark.parametrize("log_n", [18, 19])
def test_commit_by_eight_at_2p18_and_2p19(sb, oracle, log_n):
    """round 1 has 2^15 / 2^16 elements: the fold by 8 inside the leaf kernel.  (No model transcript here: it would pickle every leaf.)"""
    N, expansion, t, a, k = 1 << log_n, 4, 4, 8, 3
    omega = oracle.primitive_nth_root(N)
    soa = model.codeword_of(oracle, SEED + log_n, N, expansion, OFFSET, omega)
    fri = _fri(sb, N, expansion, t, a)
    cw = sb.XArray.from_numpy(soa)
    ps = sb.ProofStream()
    codewords, trees = fri.commit(cw, ps)
    F = model.num_folds(N, expansion, k)
    assert fri.num_rounds() == F + 1 == len(codewords) and len(trees) == F
    assert [len(c) for c in codewords] == [N >> (k * r) for r in range(F + 1)]
    host = [c.array.to_numpy() for c in codewords]
    assert np.array_equal(host[0], soa)
    # every tree root is the stand-alone tree's over the same codeword; roots 1 .. F are in the stream, then the last codeword
    roots = [sb.Merkle(c.array).root() for c in codewords]
    assert [tree.root() for tree in trees] == roots[:-1]
    assert [bytes(x) for x in ps.objects[:F]] == roots[1:] and len(ps.objects) == F + 1
    assert [[c.value for c in e.polynomial.coefficients] for e in ps.objects[F]] == \
        [oracle.xtrim([int(host[F][j, i]) for j in range(3)]) for i in range(host[F].shape[1])]
    # every codeword is the oracle's k-fold composition of the one before, with the challenge the transcript gives
    mirror = oracle.ProofStreamOracle()
    g, w = OFFSET, omega
    for r in range(F):
        if r > 0:
            mirror.push(roots[r])
        alpha = oracle.xsample(mirror.prover_fiat_shamir())
        want, g, w = model.fold_round(oracle, host[r], alpha, g, w, k)
        assert np.array_equal(want, host[r + 1]), "codeword %d" % (r + 1)
    root0 = roots[0]
    del codewords, trees
    ps2 = sb.ProofStream()
    top = fri.prove(cw, ps2)
    assert len(top) == t and all(0 <= i < N >> k for i in top)
    assert [bytes(x) for x in ps2.objects[:F]] == roots[1:]
    vs = sb.ProofStream()
    vs.objects = list(ps2.objects)
    assert fri.verify(vs, root0) is True and vs.read_index == len(vs.objects)


# ------------------------------------------------------------------------------------------------ 4. switches and prior state
_CHILD = r"""
import hashlib, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import stark_brainfuck_amd as sb
import test_gpu_fri_folding as T
from oracle import ref_oracle as o
N, expansion, t = 1 << 10, 4, 4
XF = sb.ExtensionField.main()
cw = T.model.codeword_of(o, T.SEED + N + expansion, N, expansion, T.OFFSET, o.primitive_nth_root(N))
for a in (None, 2):
    for pre in (False, True):
        ps = sb.ProofStream()
        if pre:
            for obj in T._prepushed(XF.from_limbs, o):
                ps.push(obj)
        top = T._fri(sb, N, expansion, t, a, XF).prove(sb.XArray.from_numpy(cw), ps)
        print("RESULT", a, pre, top, hashlib.sha256(ps.serialize()).hexdigest())
"""


def _child(lookahead):
    env = dict(os.environ)
    env.pop("BFS_FRI_LOOKAHEAD", None)
    if lookahead is not None:
        env["BFS_FRI_LOOKAHEAD"] = lookahead
    res = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:]
    return [line for line in res.stdout.splitlines() if line.startswith("RESULT")]


def test_folding_by_two_is_the_default_with_and_without_the_lookahead(sb):
    """the look-ahead switch is read once per process, so each setting gets a process of its own: BFS_FRI_LOOKAHEAD unset and = 0.
    Fri(...) and Fri(..., folding_factor=2) write the same bytes, and they are the reference's (= the model's for a = 2)."""
    N, expansion, t = 1 << 10, 4, 4
    want = []
    for a in (None, 2):
        for pre in (False, True):
            ref = _reference(N, expansion, t, 2, prepushed=pre)
            want.append("RESULT %s %s %s %s" % (a, pre, ref["indices"], hashlib.sha256(ref["bytes"]).hexdigest()))
    assert _child(None) == want
    assert _child("0") == want


@pytest.mark.parametrize("a,N", [(4, 1 << 10), (8, 1 << 11), (4, 1 << 17)])
def test_prove_behind_objects_pushed_beforehand(sb, oracle, a, N):
    """the stream already holds objects (6.5 KB of them: the Fiat-Shamir look-ahead engages and has to count F - 1 coming roots)"""
    expansion, t = 4, 4
    ref = _reference(N, expansion, t, a, prepushed=True)
    XF = sb.ExtensionField.main()
    ps = sb.ProofStream()
    pre = _prepushed(XF.from_limbs, oracle)
    for obj in pre:
        ps.push(obj)
    fri = _fri(sb, N, expansion, t, a, XF)
    assert fri.prove(sb.XArray.from_numpy(ref["codeword"]), ps) == ref["indices"]
    assert ps.serialize() == ref["bytes"]
    vs = sb.ProofStream()
    vs.objects, vs.read_index = list(ps.objects), len(pre)
    assert fri.verify(vs, ref["roots"][0]) is True


# ------------------------------------------------------------------------------------------------ 5. argument checks
def test_set_folding_argument_checks(sb, oracle):
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.ip import NativeTranscript
    lib = _lib.load()
    N, expansion = 64, 4
    omega = oracle.primitive_nth_root(N)
    cw = sb.XArray.from_numpy(model.codeword_of(oracle, SEED, N, expansion, OFFSET, omega))
    session = lib.bfs_fri_session_new()
    try:
        for bad in (0, 4, 5, 2 ** 32 - 1):
            assert lib.bfs_fri_session_set_folding(session, bad) == BFS_ERR_BAD_ARG
            assert b"log2_folding" in lib.bfs_last_error()
        for good in (1, 3, 2):
            assert lib.bfs_fri_session_set_folding(session, good) == 0
        transcript = NativeTranscript()
        _lib.check(lib.bfs_fri_commit(session, transcript.handle, cw.ptr, cw.stride, 6, OFFSET, omega, expansion, 0))
        assert lib.bfs_fri_session_rounds(session) == 2          # L = 4, k = 2: one fold
        assert lib.bfs_fri_session_set_folding(session, 1) == BFS_ERR_BAD_ARG
        assert b"already committed" in lib.bfs_last_error()
    finally:
        lib.bfs_fri_session_free(session)
    # too few halvings for one fold by 8; a fold of a codeword shorter than the factor
    session = lib.bfs_fri_session_new()
    try:
        assert lib.bfs_fri_session_set_folding(session, 3) == 0
        transcript = NativeTranscript()
        assert lib.bfs_fri_commit(session, transcript.handle, cw.ptr, cw.stride, 6, OFFSET, omega, 16, 0) == BFS_ERR_BAD_ARG
    finally:
        lib.bfs_fri_session_free(session)
    out = sb.XArray.from_numpy(np.zeros((3, 8), dtype=np.uint64))
    alpha = (ctypes.c_uint64 * 3)(1, 2, 3)
    assert lib.bfs_xfe_fold_multi(cw.ptr, cw.stride, out.ptr, 8, 2, 3, alpha, OFFSET, oracle.primitive_nth_root(4), 0) == BFS_ERR_BAD_ARG
    assert lib.bfs_xfe_fold_multi(cw.ptr, cw.stride, out.ptr, 8, 6, 0, alpha, OFFSET, omega, 0) == BFS_ERR_BAD_ARG
    assert lib.bfs_xfe_fold_multi(cw.ptr, cw.stride, out.ptr, 8, 6, 4, alpha, OFFSET, omega, 0) == BFS_ERR_BAD_ARG
    assert lib.bfs_xfe_fold_multi(cw.ptr, cw.stride, out.ptr, 4, 6, 3, alpha, OFFSET, omega, 0) == BFS_ERR_BAD_ARG       # out_stride < n / 8
