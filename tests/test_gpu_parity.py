"""Parity tests proper: the HIP path (through the C ABI / the Python mirror) against the CPU oracle on the same
seeded inputs, against the golden fixtures captured from the reference, and -- at BASELINE.json's full sizes --
through size-independent properties.  Everything here needs the MI355X (`-m gpu`).  Bit-exact throughout: the
path is integer arithmetic mod p and byte hashing; there is no tolerance."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden_bytes, load_golden

pytestmark = pytest.mark.gpu
SEED = 0x5EED
P = (1 << 64) - (1 << 32) + 1


@pytest.fixture(scope="module")
def sb():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import stark_brainfuck_amd
    from stark_brainfuck_amd import _lib
    _lib.load()            # raises BackendUnavailable if the HIP library is missing: no fallback
    return stark_brainfuck_amd


def sha_u64(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<u8").tobytes()).hexdigest()


def addmod(a, b):
    """(a + b) mod p on uint64 arrays of canonical residues."""
    P, EPS = np.uint64(0xFFFFFFFF00000001), np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        s = a + b
        return np.where(s < a, s + EPS, np.where(s >= P, s - P, s))


def raw_ntt(sb, v, logn, root, shift=1, scale=1, n_in=None, batch=1):
    """straight through the C ABI: bfs_gl_ntt on device buffers."""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer, synchronize
    n = 1 << logn
    n_in = n if n_in is None else n_in
    din, dout = DeviceBuffer.from_numpy(v), DeviceBuffer(n * batch)
    _lib.check(_lib.load().bfs_gl_ntt(din.ptr, n_in, n_in, dout.ptr, n, logn, batch, root, shift, scale, 0))
    synchronize(0)
    return dout.to_numpy()


@pytest.mark.parametrize("logn", [6, 9, 12, 13, 16, 17, 20, 22, 24])
def test_zero_padded_transforms_of_every_fill(sb, oracle, logn):
    """fast_coset_evaluate of d coefficients on n points (ntt.py:164-168) for d around n/64, n/16, n/8, n/4, n/2 -- the shapes Table.lde makes
    (table.py:138-149).  The first register stage knows how many of its 16 registers can be non-zero and runs the network for those only
    (ntt_core.hpp: dif_sparse -- 1, 2, 4 or 8 live inputs); values next to 0 and p ride along in the last column."""
    n = 1 << logn
    w = oracle.primitive_nth_root(n)
    v = oracle.felt_array(SEED + 17 * logn, 0, n)
    P = (1 << 64) - (1 << 32) + 1
    edge = np.array([0, 1, P - 1, P - 2, 2, (1 << 32) - 1, 1 << 32, P - (1 << 32)] * (n // 8 if n >= 8 else 1), dtype=np.uint64)[:n]
    counts = sorted({1, max(1, n // 64), n // 16, n // 16 + 1, n // 8, n // 8 + 1, n // 4 + 1, n // 2, n // 2 + 3} & set(range(1, n + 1)))
    if logn >= 22:
        counts = [c for c in counts if c in (n // 64, n // 16 + 1, n // 8, n // 2)]
    for d in counts:
        for shift in ((7,) if logn >= 20 else (1, 7)):
            for src in (v, edge):
                assert (raw_ntt(sb, src[:d], logn, w, shift, 1, n_in=d) == oracle.fast_coset_evaluate(src[:d], shift, w, n)).all(), (logn, d, shift)


# ------------------------------------------------------------------------------------------------ NTT
@pytest.mark.parametrize("logn", list(range(0, 24)))
def test_ntt_intt_coset_vs_oracle(sb, oracle, logn):
    n = 1 << logn
    v = oracle.felt_array(SEED, 0, n)
    w = oracle.primitive_nth_root(n)
    assert (raw_ntt(sb, v, logn, w) == oracle.ntt(w, v)).all()
    assert (raw_ntt(sb, v, logn, oracle.inv(w), 1, oracle.inv(n)) == oracle.intt(w, v)).all()
    d = max(1, n // 4)
    assert (raw_ntt(sb, v[:d], logn, w, 7, 1, n_in=d) == oracle.fast_coset_evaluate(v[:d], 7, w, n)).all()


def edge_values(n, seed):
    """values next to 0, next to p and around 2^32, a few random ones: what trace columns look like, and what makes an unreduced
    butterfly sum (gl.hpp: gl_add_lazy) actually exceed p -- random operands do that once in 2^32 (tests/test_emulation.py has the
    same generator and also counts non-canonical operands inside the emulated kernels)"""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 6, n, dtype=np.uint64)
    kind = rng.integers(0, 8, n)
    v = np.where(kind < 3, small, np.uint64(P) - np.uint64(1) - small)
    v = np.where(kind == 6, rng.integers(0, P, n, dtype=np.uint64), v)
    v = np.where(kind == 7, (np.uint64(1) << np.uint64(32)) - small, v)
    return np.ascontiguousarray(v, dtype=np.uint64)


@pytest.mark.parametrize("logn", list(range(1, 25)))
def test_ntt_on_values_next_to_zero_and_p(sb, oracle, logn):
    """every plan shape on inputs next to 0 and p: forward, inverse, coset and plain zero-padded transforms equal the oracle's bit
    for bit -- in particular every output is a canonical residue.  Such inputs drive the unreduced sums over p in the FIRST butterfly
    block of the first pass only: after the first inner twiddle the operands are uniform again.  The later stages and passes meet
    operands of this kind in tests/test_gpu_ntt_planted.py, whose inputs are computed to put them there.  (Round 4: a first version
    of the lazy sums passed every random-data test and put a value >= p into a proof's codeword.)"""
    n = 1 << logn
    w = oracle.primitive_nth_root(n)
    for seed in range(3 if logn <= 16 else 1):
        v = edge_values(n, 1000 * logn + seed)
        assert (raw_ntt(sb, v, logn, w) == oracle.ntt(w, v)).all(), seed
        assert (raw_ntt(sb, v, logn, oracle.inv(w), 1, oracle.inv(n)) == oracle.intt(w, v)).all(), seed
        d = max(1, n // 4)
        assert (raw_ntt(sb, v[:d], logn, w, 7, 1, n_in=d) == oracle.fast_coset_evaluate(v[:d], 7, w, n)).all(), seed
        assert (raw_ntt(sb, v[:d], logn, w, 1, 1, n_in=d) == oracle.fast_coset_evaluate(v[:d], 1, w, n)).all(), seed
    # all-(p - 1) and alternating 1 / p - 1 columns: sums of exactly p and 2p - 2 at the first level
    special = (np.full(n, P - 1, dtype=np.uint64), np.where(np.arange(n) % 2 == 0, np.uint64(1), np.uint64(P - 1)).astype(np.uint64))
    want = [oracle.ntt(w, v) for v in special]
    for v, f in zip(special, want):
        assert (raw_ntt(sb, v, logn, w) == f).all()
    if logn >= 23:
        # the bench shape (8 + 8 + 7 and 8 + 8 + 8 bits, round-4 verdict: edge values stopped at 2^22): above 128 MiB per call the kernels
        # are the non-temporal instantiations, which a single column never reaches -- the same columns again as ONE batched call
        v = edge_values(n, 1000 * logn)
        batch = np.concatenate([v, special[0], special[1]])
        got = raw_ntt(sb, batch, logn, w, batch=3).reshape(3, n)
        assert (got[0] == oracle.ntt(w, v)).all() and (got[1] == want[0]).all() and (got[2] == want[1]).all()
        got = raw_ntt(sb, batch, logn, oracle.inv(w), 1, oracle.inv(n), batch=3).reshape(3, n)
        assert (got[0] == oracle.intt(w, v)).all()


@pytest.mark.parametrize("logn", [1, 4, 7, 10, 13, 16])
def test_elementwise_primitives_on_values_next_to_zero_and_p(sb, oracle, logn):
    """the same edge operands through the other arithmetic entry points: Polynomial.scale, the pointwise product, the batch inverse and
    one split-and-fold round (unreduced dot products, lazy.hpp) -- against the oracle, bit for bit"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer, synchronize
    lib = _lib.load()
    n = 1 << logn
    a, b = edge_values(n, 7 * logn + 1), edge_values(n, 7 * logn + 2)
    da, db, dout = DeviceBuffer.from_numpy(a), DeviceBuffer.from_numpy(b), DeviceBuffer(n)
    for factor in (1, 2, P - 1, P - 2, (1 << 32) - 1, 1 << 32, oracle.felt(SEED, logn)):
        _lib.check(lib.bfs_gl_scale(da.ptr, dout.ptr, n, n, 1, factor, 0)); synchronize(0)
        assert (dout.to_numpy() == oracle.scale(factor, a)).all(), factor
    _lib.check(lib.bfs_gl_mul_pointwise(da.ptr, db.ptr, dout.ptr, n, 0)); synchronize(0)
    assert (dout.to_numpy() == oracle.hadamard(a, b)).all()
    nz = np.where(a == 0, np.uint64(P - 1), a)
    dnz = DeviceBuffer.from_numpy(nz)
    _lib.check(lib.bfs_gl_batch_inverse(dnz.ptr, dout.ptr, n, 0)); synchronize(0)
    assert (dout.to_numpy() == oracle.batch_inverse(nz)).all()
    if logn >= 1:
        soa = np.stack([edge_values(n, 7 * logn + 3 + k) for k in range(3)])
        dcw, dfold = DeviceBuffer.from_numpy(np.ascontiguousarray(soa.reshape(-1))), DeviceBuffer(3 * (n // 2))
        omega = oracle.primitive_nth_root(n)
        for alpha in ((P - 1, P - 1, P - 1), (1, 0, 0), (0, P - 1, 1), tuple(oracle.felt(SEED + 5, 3 * logn + k) for k in range(3))):
            for offset in (1, 7, P - 1):
                _lib.check(lib.bfs_xfe_fold(dcw.ptr, n, dfold.ptr, n // 2, logn, (ctypes.c_uint64 * 3)(*alpha), offset, omega, 0)); synchronize(0)
                assert (dfold.to_numpy().reshape(3, -1) == oracle.fri_fold(soa, alpha, offset, omega)).all(), (alpha, offset)


def test_ntt_golden_vectors(sb):
    g = load_golden("ntt.json")
    import oracle.ref_oracle as o
    for logn, c in g["cases"].items():
        n = 1 << int(logn)
        v = o.felt_array(SEED, 0, n)
        fw = raw_ntt(sb, v, int(logn), c["root"])
        assert sha_u64(fw) == c["sha_ntt"], logn
        if "ntt" in c:
            assert fw.tolist() == c["ntt"]
        if n > 1:
            iv = raw_ntt(sb, v, int(logn), o.inv(c["root"]), 1, o.inv(n))
            assert sha_u64(iv) == c["sha_intt"], logn


def test_config2_2p20_forward_inverse_golden(sb, oracle):
    """BASELINE config 2: 2^20-point forward + inverse NTT, bit-exact vs the reference's ntt.py (ntt20.json)."""
    c = load_golden("ntt20.json")
    v = oracle.felt_array(SEED, 0, 1 << 20)
    assert sha_u64(v) == c["sha_in"]
    fw = raw_ntt(sb, v, 20, c["root"])
    assert sha_u64(fw) == c["sha_ntt"] and fw[:4].tolist() == c["ntt_head"] and fw[-4:].tolist() == c["ntt_tail"]
    iv = raw_ntt(sb, v, 20, oracle.inv(c["root"]), 1, oracle.inv(1 << 20))
    assert sha_u64(iv) == c["sha_intt"]
    assert (raw_ntt(sb, fw, 20, oracle.inv(c["root"]), 1, oracle.inv(1 << 20)) == v).all()


def test_config5_2p24_columns(sb, oracle):
    """BASELINE config 5: eight 2^24-point columns (column c = felt(seed + c * 2^32, i)) in one batched call.
    Every column's SHA-256 against the oracle's known answers (tests/golden/ntt24_oracle.json, made by gen_ntt24_oracle.py),
    columns 0 and 5 against the oracle run live on this box, then the size-independent properties on the whole batch:
    inverse round trip and linearity.  The same columns one at a time must give the same bytes (the sharded layout)."""
    g = load_golden("ntt24_oracle.json")
    logn, n, cols = 24, 1 << 24, 8
    assert g["log_n"] == logn and len(g["columns"]) == cols
    w = oracle.primitive_nth_root(n)
    assert w == g["root"]
    v = np.concatenate([oracle.felt_array(SEED + (c << 32), 0, n) for c in range(cols)])
    fw = raw_ntt(sb, v, logn, w, batch=cols)
    for c in range(cols):
        assert sha_u64(v[c * n:(c + 1) * n]) == g["columns"][c]["input_sha256"], c
        assert sha_u64(fw[c * n:(c + 1) * n]) == g["columns"][c]["output_sha256"], c
        assert [int(x) for x in fw[c * n:c * n + 3]] == g["columns"][c]["output_head"]
    for c in (0, 5):
        assert (fw[c * n:(c + 1) * n] == oracle.ntt(w, v[c * n:(c + 1) * n])).all(), c
    back = raw_ntt(sb, fw, logn, oracle.inv(w), 1, oracle.inv(n), batch=cols)
    assert (back == v).all()
    # linearity: NTT(a + b) = NTT(a) + NTT(b) (mod p), on column pairs (1, 2), (3, 4), (6, 7)
    for a, b in ((1, 2), (3, 4), (6, 7)):
        assert (raw_ntt(sb, addmod(v[a * n:(a + 1) * n], v[b * n:(b + 1) * n]), logn, w) == addmod(fw[a * n:(a + 1) * n], fw[b * n:(b + 1) * n])).all()
    # a column transformed on its own (what a rank of the sharded run does) is the same bytes as inside the batch
    for c in (3, 7):
        assert sha_u64(raw_ntt(sb, v[c * n:(c + 1) * n], logn, w)) == g["columns"][c]["output_sha256"]


@pytest.mark.parametrize("route", ["direct", "buffer0", "buffer2", "tune", "auto"])
def test_large_transform_over_every_route(route):
    """A transform of >= 256 MiB can write its first pass straight into the output or through one of three library buffers (ntt.hip).
    Each route forced in a process of its own (BFS_NTT_WS_PROBE is read once); "tune": the explicit bfs_ntt_tune call of round 5 on the
    pair, after which bfs_gl_ntt takes the remembered route; "auto": the round-4 behaviour behind BFS_NTT_WS_PROBE=auto (the third call
    measures).  Three 2^24 columns of the bench workload against the oracle's known answers (tests/golden/ntt24_oracle.json), four
    times, the input untouched -- and what the library keeps afterwards: at most the one buffer it chose; nothing at all once the pair
    is forgotten or one of its buffers goes back to the pool."""
    import subprocess
    import sys
    code = r'''
import sys, json, hashlib, os
sys.path.insert(0, %r)
import numpy as np
from oracle import ref_oracle as o
from stark_brainfuck_amd import _lib
from stark_brainfuck_amd.device import DeviceBuffer, synchronize
lib = _lib.load()
g = json.load(open(%r))
logn, n, cols = 24, 1 << 24, 3
v = np.concatenate([o.felt_array(0x5EED + (c << 32), 0, n) for c in range(cols)])
din, dout = DeviceBuffer.from_numpy(v), DeviceBuffer(n * cols)
import ctypes
hip = ctypes.CDLL("libamdhip64.so")
def free_bytes():
    f, t = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
    return f.value
def probes():
    k = ctypes.c_ulonglong(0)
    _lib.check(lib.bfs_ntt_route_probe_info(None, None, ctypes.byref(k)))
    return k.value
_lib.check(lib.bfs_gl_ntt(din.ptr, n, n, dout.ptr, n, logn, cols, g["root"], 1, 1, 0)); synchronize(0)      # tables exist from here on
before = free_bytes()
mode = %r
chosen = ctypes.c_int(-7)
if mode == "tune":
    _lib.check(lib.bfs_ntt_tune(din.ptr, n, dout.ptr, n, logn, cols, g["root"], 0, ctypes.byref(chosen)))
    assert probes() == 1 and -1 <= chosen.value <= 2
for rep in range(4):
    _lib.check(lib.bfs_memset(dout.ptr, 0, 8 * n * cols, 0))
    _lib.check(lib.bfs_gl_ntt(din.ptr, n, n, dout.ptr, n, logn, cols, g["root"], 1, 1, 0)); synchronize(0)
    out = dout.to_numpy()
    for c in range(cols):
        assert hashlib.sha256(np.ascontiguousarray(out[c * n:(c + 1) * n], dtype="<u8").tobytes()).hexdigest() == g["columns"][c]["output_sha256"], (rep, c)
assert (din.to_numpy() == v).all()
assert probes() == (1 if mode in ("tune", "auto") else 0)     # bfs_gl_ntt measures nothing by itself unless asked to ("auto": once, at the third call)
# at most the one candidate buffer that was chosen stays (the others went back to the driver): <= one transform's size
held = before - free_bytes()
assert held <= 8 * n * cols + (1 << 20), held
if mode == "tune":
    assert (held >= 8 * n * cols) == (chosen.value >= 0), (held, chosen.value)
    # a pair dies with either of its buffers: the output goes back to the pool, a new buffer takes its address, the route is gone
    gone = ctypes.c_size_t(99)
    dout.free(); dout = DeviceBuffer(n * cols)
    _lib.check(lib.bfs_ntt_route_forget(None, ctypes.byref(gone)))
    assert gone.value == 0, gone.value                        # (already forgotten when the block was released)
    _lib.check(lib.bfs_pool_trim())
    dout = None
if mode in ("tune", "auto"):
    _lib.check(lib.bfs_ntt_route_forget(None, None))
    din = dout = None
    _lib.check(lib.bfs_pool_trim())
    assert free_bytes() >= before + 8 * n * cols * 2 - (1 << 20), (free_bytes(), before)      # candidates AND the two data buffers are back
print("ok")
''' % (ROOT, os.path.join(GOLDEN, "ntt24_oracle.json"), route)
    env = dict(os.environ, BFS_NTT_WS_PROBE_LOG="1")
    env.pop("BFS_NTT_WS_PROBE", None)
    if route not in ("tune",):
        env["BFS_NTT_WS_PROBE"] = route
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and "ok" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]
    assert res.stderr.count("bfs ntt route") == (1 if route in ("tune", "auto") else 0)


def test_ntt_tune_without_room_for_its_candidates_leaves_nothing_behind():
    """bfs_ntt_tune with less than four transform sizes of free memory: the pair stays on the direct route, no candidate buffer and no
    event survives the call (round-4 advice: the hidden measurement leaked its events on early returns and spiked memory), and the
    call refuses a stream that is being captured."""
    import subprocess
    import sys
    code = r'''
import sys, ctypes
sys.path.insert(0, %r)
import numpy as np
from stark_brainfuck_amd import _lib
from stark_brainfuck_amd.device import DeviceBuffer, synchronize
lib = _lib.load()
hip = ctypes.CDLL("libamdhip64.so")
def free_bytes():
    f, t = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
    return f.value
logn, n, cols = 24, 1 << 24, 3
root = lib.bfs_gl_primitive_root(logn)
din, dout = DeviceBuffer(n * cols), DeviceBuffer(n * cols)
_lib.check(lib.bfs_memset(din.ptr, 1, 8 * n * cols, 0))
_lib.check(lib.bfs_gl_ntt(din.ptr, n, n, dout.ptr, n, logn, cols, root, 1, 1, 0)); synchronize(0)
size = 8 * n * cols
ballast = ctypes.c_void_p()
take = free_bytes() - 3 * size                # leaves three transform sizes: enough for the candidates themselves, not for the margin
assert hip.hipMalloc(ctypes.byref(ballast), ctypes.c_size_t(take)) == 0
before = free_bytes()
r = ctypes.c_int(5)
_lib.check(lib.bfs_ntt_tune(din.ptr, n, dout.ptr, n, logn, cols, root, 0, ctypes.byref(r)))
assert r.value == -1
k = ctypes.c_ulonglong(7)
_lib.check(lib.bfs_ntt_route_probe_info(None, None, ctypes.byref(k)))
assert k.value == 0 and free_bytes() == before
assert hip.hipFree(ballast) == 0
print("ok")
''' % (ROOT,)
    env = dict(os.environ, BFS_NTT_WS_PROBE_LOG="1")
    env.pop("BFS_NTT_WS_PROBE", None)
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "ok" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]
    assert "not measured (less than four transform sizes of free memory)" in res.stderr


def test_ntt_other_roots_and_batches(sb, oracle):
    for logn in (6, 11, 13, 17):
        n = 1 << logn
        w = oracle.power(oracle.primitive_nth_root(n), 3)
        v = oracle.felt_array(SEED + logn, 0, 4 * n)
        got = raw_ntt(sb, v, logn, w, batch=4).reshape(4, n)
        for b in range(4):
            assert (got[b] == oracle.ntt(w, v[b * n:(b + 1) * n])).all()


def test_ntt_error_behaviour(sb):
    g = load_golden("ntt.json")["errors"]
    F = sb.BaseField.main()
    w8 = F.primitive_nth_root(8)
    with pytest.raises(AssertionError) as e:
        sb.ntt(w8, [F(1)] * 6)
    assert str(e.value) == g["non_pow2"]
    with pytest.raises(AssertionError) as e:
        sb.ntt(F(3), [F(1)] * 8)
    assert str(e.value) == g["not_root"]
    with pytest.raises(AssertionError) as e:
        sb.ntt(F.primitive_nth_root(4), [F(1)] * 8)
    assert str(e.value).startswith("primitive root 281474976710656 is not primitive nth root of unity, where n is 8")
    with pytest.raises(AssertionError) as e:
        sb.intt(w8, [F(1)] * 6)
    assert str(e.value) == g["intt_non_pow2"]
    with pytest.raises(AssertionError) as e:
        sb.intt(F(3), [F(1)] * 8)
    assert str(e.value) == g["intt_not_root"]
    one = [F(5)]
    assert sb.ntt(w8, one) is one            # ntt.py:8-9 returns its argument for length <= 1


# ---- the reference's own test_ntt.py, restated against this API (object lists in, object lists out)
def test_reference_test_ntt(sb):
    F = sb.BaseField.main()
    n = 1 << 8
    w = F.primitive_nth_root(n)
    coeffs = [F.sample(os.urandom(17)) for _ in range(n)]
    values = sb.ntt(w, coeffs)
    assert values == sb.Polynomial(coeffs).evaluate_domain([w ^ i for i in range(n)])


def test_reference_test_intt(sb):
    F = sb.BaseField.main()
    for logn in range(1, 8):
        n = 1 << logn
        w = F.primitive_nth_root(n)
        values = [F.sample(os.urandom(1)) for _ in range(n)]
        coeffs = sb.intt(w, values)
        assert sb.ntt(w, coeffs) == values
        poly = sb.Polynomial(coeffs)
        assert [poly.evaluate(w ^ i) for i in range(n)] == values


def test_reference_test_multiply_and_divide(sb):
    F = sb.BaseField.main()
    n = 64
    w = F.primitive_nth_root(n)
    for _ in range(20):
        ld, rd = os.urandom(1)[0] % (n // 2), os.urandom(1)[0] % (n // 2)
        lhs = sb.Polynomial([F.sample(os.urandom(17)) for _ in range(ld + 1)])
        rhs = sb.Polynomial([F.sample(os.urandom(17)) for _ in range(rd + 1)])
        prod = sb.fast_multiply(lhs, rhs, w, n)
        assert prod == lhs * rhs
        assert sb.fast_coset_divide(prod, lhs, F.generator(), w, n) == rhs


def test_fast_multiply_and_coset_goldens(sb):
    g = load_golden("poly.json")
    F = sb.BaseField.main()
    w = F.primitive_nth_root(64)
    P = lambda c: sb.Polynomial([F(x) for x in c])
    for c in g["fast_multiply_n64"]:
        prod = sb.fast_multiply(P(c["lhs"]), P(c["rhs"]), w, 64)
        assert [x.value for x in prod.coefficients] == c["product"]
        if "quotient_by_lhs" in c:
            q = sb.fast_coset_divide(prod, P(c["lhs"]), F.generator(), w, 64)
            assert [x.value for x in q.coefficients] == c["quotient_by_lhs"]
    for c in g["coset"]:
        gen = F.primitive_nth_root(c["order"])
        vals = sb.fast_coset_evaluate(P(c["coefficients"]), F(c["offset"]), gen, c["order"])
        assert [x.value for x in vals] == c["values"]
        back = sb.fast_coset_interpolate(F(c["offset"]), gen, vals)
        assert [x.value for x in back.coefficients] == c["interpolated"]
    b = g["batch_inverse"]
    assert [x.value for x in sb.batch_inverse([F(x) for x in b["in"]])] == b["out"]
    with pytest.raises(AssertionError) as e:
        sb.batch_inverse([F(1), F(0)])
    assert str(e.value) == b["zero_message"]


def test_subproduct_tree_goldens_and_reference_test_interpolate(sb):
    """fast_zerofier / fast_evaluate / fast_interpolate (ntt.py:82-161) against the reference's outputs, then
    test_ntt.py:90-114 restated (smaller n)."""
    F = sb.BaseField.main()
    for c in load_golden("poly2.json")["cases"]:
        w = F.primitive_nth_root(c["root_order"])
        D, V = [F(v) for v in c["domain"]], [F(v) for v in c["values"]]
        assert [x.value for x in sb.fast_zerofier(D, w, c["root_order"]).coefficients] == c["zerofier"]
        poly = sb.fast_interpolate(D, V, w, c["root_order"])
        assert poly.degree() == c["interpolant_degree"]
        assert sb.Polynomial([F(x) for x in c["interpolant"]]) == poly
        assert [x.value for x in sb.fast_evaluate(poly, D, w, c["root_order"])] == c["evaluated_back"] == c["values"]
        assert [x.value for x in sb.fast_evaluate(sb.Polynomial([F(x) for x in c["poly"]]), D, w, c["root_order"])] == c["poly_evaluated"]
    n = 128
    w = F.primitive_nth_root(n)
    for N in (37, 64, 100):
        values = [F.sample(os.urandom(17)) for _ in range(N)]
        domain = [F.sample(os.urandom(17)) for _ in range(N)]
        poly = sb.fast_interpolate(domain, values, w, n)
        assert sb.fast_evaluate(poly, domain, w, n)[:N] == values


def _xpoly(sb, XF, limbs_list):
    return sb.Polynomial([XF.from_limbs(list(l)) for l in limbs_list])


def _xl3(e):
    c = [x.value for x in e.polynomial.coefficients]
    return c + [0] * (3 - len(c))


def test_fast_family_over_the_extension_field_goldens(sb):
    """fast_multiply / fast_coset_divide / batch_inverse / fast_zerofier / fast_evaluate / fast_interpolate on ExtensionFieldElement
    operands with a lifted root (ntt.py:45-79, 82-161, 177-235 as Table.ldex calls them, table.py:112-149) against the reference's
    own outputs (tests/golden/polyx.json)."""
    g = load_golden("polyx.json")
    XF = sb.ExtensionField.main()
    BF = XF._base()
    for c in g["fast_multiply"]:
        w = XF.lift(BF.primitive_nth_root(c["order"]))
        lhs, rhs = _xpoly(sb, XF, c["lhs"]), _xpoly(sb, XF, c["rhs"])
        prod = sb.fast_multiply(lhs, rhs, w, c["order"])
        assert [_xl3(x) for x in prod.coefficients] == c["product"]
        if "quotient_by_lhs" in c:
            q = sb.fast_coset_divide(prod, lhs, XF.lift(BF.generator()), w, c["order"])
            assert [_xl3(x) for x in q.coefficients] == c["quotient_by_lhs"]
    b = g["batch_inverse"]
    assert [_xl3(x) for x in sb.batch_inverse([XF.from_limbs(l) for l in b["in"]])] == b["out"]
    with pytest.raises(AssertionError) as e:
        sb.batch_inverse([XF.from_limbs([1, 2, 3]), XF.zero()])
    assert str(e.value) == b["zero_message"]
    for c in g["interpolate_columns"] + [dict(g["generic_points"], height=None)]:
        N = c["N"]
        w = XF.lift(BF.primitive_nth_root(N))
        D = [XF.from_limbs(l) for l in c["domain"]]
        assert [_xl3(x) for x in sb.fast_zerofier(D, w, N).coefficients] == c["zerofier"]
        poly = sb.fast_interpolate(D, [XF.from_limbs(l) for l in c["values"]], w, N)
        assert [_xl3(x) for x in poly.coefficients][:len(c["interpolant"])] == c["interpolant"]
        assert all(x.is_zero() for x in poly.coefficients[len(c["interpolant"]):])
        if c["height"] is not None:
            assert poly.degree() == c["interpolant_degree"]
            assert [_xl3(x) for x in sb.fast_evaluate(poly, D, w, N)] == c["evaluated_back"] == c["values"]
        else:
            assert [_xl3(x) for x in sb.fast_evaluate(_xpoly(sb, XF, c["poly"]), D, w, N)] == c["poly_evaluated"]


def test_roots_and_offsets_outside_the_base_field_goldens(sb):
    """ntt.py's call surface with arguments that do not come from the base field (tests/golden/polyxo.json, the reference's outputs): a
    genuine extension element is never a 2^k-th root of unity (the 2-part of p^3 - 1 is that of p - 1), so every transform meets the
    reference's own assertion, message for message; a coset OFFSET may be any extension element, and fast_coset_evaluate / _interpolate /
    _divide give the reference's values."""
    import hashlib
    import struct
    g = load_golden("polyxo.json")
    XF = sb.ExtensionField.main()
    BF = XF._base()
    e = g["extension_root"]
    bad = XF.from_limbs(e["root"])
    vals = [XF.from_limbs(l) for l in e["values"]]
    w8 = XF.lift(BF.primitive_nth_root(8))
    assert [_xl3(x) for x in sb.ntt(w8, vals)] == e["lifted_root_values_ntt"]
    for name, call in (("ntt", lambda: sb.ntt(bad, vals)), ("intt", lambda: sb.intt(bad, vals)),
                       ("fast_multiply", lambda: sb.fast_multiply(sb.Polynomial(vals), sb.Polynomial(vals), bad, 16)),
                       ("fast_coset_divide", lambda: sb.fast_coset_divide(sb.Polynomial(vals), sb.Polynomial(vals[:3]), w8, bad, 16))):
        with pytest.raises(AssertionError) as info:
            call()
        assert str(info.value) == e[name], name
    for c in g["extension_offset"]:
        n = c["order"]
        w = XF.lift(BF.primitive_nth_root(n))
        offset = XF.from_limbs(c["offset"])
        poly = _xpoly(sb, XF, c["poly"])
        values = sb.fast_coset_evaluate(poly, offset, w, n)
        l3 = [_xl3(v) for v in values]
        h = hashlib.sha256()
        for k in range(3):
            h.update(struct.pack("<%dQ" % n, *[t[k] for t in l3]))
        assert l3[:4] == c["values_head"] and h.hexdigest() == c["values_sha"], n
        back = sb.fast_coset_interpolate(offset, w, values)
        got = [_xl3(x) for x in back.coefficients]
        assert got[:len(c["interpolated_back"])] == c["interpolated_back"] and not any(any(t) for t in got[len(c["interpolated_back"]):])
        if "quotient" in c:
            q = sb.fast_coset_divide(_xpoly(sb, XF, c["product"]), _xpoly(sb, XF, c["divisor"]), offset, w, n)
            assert [_xl3(x) for x in q.coefficients] == c["quotient"]


def test_interpolate_columns_shape_through_the_reference_call(sb):
    """Table.interpolate_columns of the reference (table.py:112-136) written out against this package: omicron powers plus one odd
    power of omega, lifted; the interpolant must agree with the rank-one form the prover uses (bfs_poly_randomize)."""
    XF = sb.ExtensionField.main()
    BF = XF._base()
    rng = np.random.default_rng(7)
    for (N, height) in [(256, 32), (1024, 64), (4096, 256)]:
        omega, omicron = BF.primitive_nth_root(N), BF.primitive_nth_root(height)
        domain = [XF.lift(omicron ^ i) for i in range(height)] + [XF.lift(omega)]
        values = [XF.from_limbs([int(v) for v in rng.integers(0, P, 3, dtype=np.uint64)]) for _ in range(height + 1)]
        poly = sb.fast_interpolate(domain, values, XF.lift(omega), N)
        assert poly.degree() <= height
        assert all(poly.evaluate(d) == v for d, v in zip(domain, values))
        # f = f0 + c (X^h - 1) with f0 = intt of the trace values over <omicron>
        f0 = sb.intt(XF.lift(omicron), values[:height])
        x = XF.lift(omega)
        c = (values[height] - sb.Polynomial(f0).evaluate(x)) / ((x ^ height) - XF.one())
        expect = list(f0) + [XF.zero()]
        expect[0] = expect[0] - c
        expect[height] = expect[height] + c
        assert sb.Polynomial(expect) == poly


@pytest.mark.parametrize("n", [1, 2, 7, 255, 256, 2047, 2048, 2049, 100003, (1 << 20) + 5])
def test_extension_field_pointwise_through_the_c_abi(sb, oracle, n):
    """bfs_xfe_mul_pointwise / bfs_xfe_batch_inverse against the oracle: ragged sizes, strided planes, in place, operands next to 0 and p"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer, synchronize
    lib = _lib.load()
    stride = n + 5
    rng = np.random.default_rng(n)
    a = np.zeros((3, stride), dtype=np.uint64)
    b = np.zeros((3, stride), dtype=np.uint64)
    for k in range(3):
        a[k, :n] = edge_values(n, 3 * n + k) if n % 2 else oracle.felt_array(SEED + k, n, n)
        b[k, :n] = edge_values(n, 5 * n + k)
    b[0, :n] = np.where((b[0, :n] | b[1, :n] | b[2, :n]) == 0, np.uint64(1), b[0, :n])      # no zero elements
    da, db, dout = DeviceBuffer.from_numpy(a.reshape(-1)), DeviceBuffer.from_numpy(b.reshape(-1)), DeviceBuffer(3 * n)
    _lib.check(lib.bfs_xfe_mul_pointwise(da.ptr, stride, db.ptr, stride, dout.ptr, n, n, 0))
    synchronize(0)
    want = oracle.xhadamard(a[:, :n], b[:, :n])
    assert (dout.to_numpy(3 * n).reshape(3, n) == want).all()
    _lib.check(lib.bfs_xfe_batch_inverse(db.ptr, stride, dout.ptr, n, n, 0))
    inv = dout.to_numpy(3 * n).reshape(3, n)
    if n <= 3000:
        assert (inv == oracle.xbatch_inverse(b[:, :n])).all()
    one = oracle.xhadamard(inv, b[:, :n])
    assert (one[0] == 1).all() and not one[1:].any()
    # in place, strided on both sides
    _lib.check(lib.bfs_xfe_batch_inverse(db.ptr, stride, db.ptr, stride, n, 0))
    _lib.check(lib.bfs_xfe_mul_pointwise(da.ptr, stride, db.ptr, stride, da.ptr, stride, n, 0))
    synchronize(0)
    got = da.to_numpy(3 * stride).reshape(3, stride)
    assert (got[:, :n] == oracle.xhadamard(a[:, :n], inv)).all() and not got[:, n:].any()
    # a zero element: the reference's assert (ntt.py:178-179), and inverse(0) = 0 in its place
    z = b[:, :n].copy()
    z[:, n // 2] = 0
    dz = DeviceBuffer.from_numpy(z.reshape(-1))
    assert lib.bfs_xfe_batch_inverse(dz.ptr, n, dz.ptr, n, n, 0) == 5
    assert "zero" in lib.bfs_last_error().decode()
    back = dz.to_numpy(3 * n).reshape(3, n)
    assert not back[:, n // 2].any()
    keep = np.arange(n) != n // 2
    assert (back[:, keep] == inv[:, keep]).all()


def test_fast_multiply_over_the_extension_field_vs_oracle(sb, oracle):
    """sizes the goldens do not reach: every halving of the root order, products up to degree 2^13"""
    XF = sb.ExtensionField.main()
    BF = XF._base()
    rng = np.random.default_rng(11)
    for (order, dl, dr) in [(1 << 14, 4000, 4100), (1 << 14, 100, 28), (1 << 10, 511, 512), (1 << 12, 3000, 9)]:
        lc = [[int(v) for v in rng.integers(0, P, 3, dtype=np.uint64)] for _ in range(dl + 1)]
        rc = [[int(v) for v in rng.integers(0, P, 3, dtype=np.uint64)] for _ in range(dr + 1)]
        w = oracle.primitive_nth_root(order)
        prod = sb.fast_multiply(_xpoly(sb, XF, lc), _xpoly(sb, XF, rc), XF.lift(BF(w)), order)
        want = oracle.xfast_multiply(lc, rc, w, order)
        assert [_xl3(x) for x in prod.coefficients] == want
        q = sb.fast_coset_divide(prod, _xpoly(sb, XF, rc), XF.lift(BF.generator()), XF.lift(BF(w)), order)
        assert [_xl3(x) for x in q.coefficients] == lc == oracle.xfast_coset_divide(want, rc, 7, w, order)
    # a base-field polynomial next to an extension one (lifted on the way in)
    F = sb.BaseField.main()
    lhs = sb.Polynomial([F(int(v)) for v in rng.integers(0, P, 20, dtype=np.uint64)])
    rhs = _xpoly(sb, XF, [[int(v) for v in rng.integers(0, P, 3, dtype=np.uint64)] for _ in range(30)])
    w = oracle.primitive_nth_root(64)
    prod = sb.fast_multiply(rhs, lhs, XF.lift(BF(w)), 64)
    want = oracle.xfast_multiply([_xl3(x) for x in rhs.coefficients], [[x.value, 0, 0] for x in lhs.coefficients], w, 64)
    assert [_xl3(x) for x in prod.coefficients] == want


def test_reference_test_coset_evaluate_and_batch_inverse(sb):
    F = sb.BaseField.main()
    n = 512
    w = F.primitive_nth_root(n)
    two = F(2)
    degree = ((os.urandom(1)[0] * 256 + os.urandom(1)[0]) % n) - 1
    poly = sb.Polynomial([F.sample(os.urandom(17)) for _ in range(degree + 1)])
    fast = sb.fast_coset_evaluate(poly, two, w, n)
    assert all(f == poly.evaluate(two * (w ^ i)) for i, f in enumerate(fast))
    arr = [F.sample(os.urandom(8)) for _ in range(100)]
    arr = [a if not a.is_zero() else F(1) for a in arr]
    assert all((i * a) == F.one() for i, a in zip(sb.batch_inverse(arr), arr))


def test_domain_and_extension_transforms(sb):
    g = load_golden("poly.json")["domain64"]
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    dom = sb.Fri.Domain(BF.generator(), BF.primitive_nth_root(64), 64)
    assert dom(5).value == g["call_5"] and [e.value for e in dom.list()[:4]] == g["list_head"]
    ev = dom.evaluate(sb.Polynomial([BF(v) for v in g["coefficients"]]))
    assert [e.value for e in ev] == g["evaluate"]
    assert [c.value for c in dom.interpolate(ev).coefficients] == g["interpolate"]
    xev = dom.xevaluate(sb.Polynomial([XF.from_limbs(l) for l in g["xcoefficients"]]))
    assert [e.limbs() for e in xev] == g["xevaluate"]
    assert [c.limbs() for c in dom.xinterpolate(xev).coefficients] == g["xinterpolate"]
    x = load_golden("ntt.json")["xfe_ntt_64"]
    w = XF.lift(BF.primitive_nth_root(64))
    vals = [XF.from_limbs(l) for l in x["in"]]
    assert [e.limbs() for e in sb.ntt(w, vals)] == x["ntt"]
    assert [e.limbs() for e in sb.intt(w, vals)] == x["intt"]


# ------------------------------------------------------------------------------------------------ Merkle
def test_merkle_goldens(sb, oracle):
    g = load_golden("merkle.json")
    XF = sb.ExtensionField.main()
    for t in g["xfe_trees"]:
        n = t["n"]
        leaves = [XF.from_limbs([oracle.felt(SEED + t["seed_offset"], 3 * i + k) for k in range(3)]) for i in range(n)]
        tree = sb.Merkle(leaves)
        assert (tree.num_leafs, tree.depth) == (n, t["depth"])
        assert tree.root().hex() == t["root"]
        assert [x.hex() for x in tree.nodes] == t["nodes"]
        for i in range(n):
            path = tree.open(i)
            assert [x.hex() for x in path] == t["paths"][i]
            assert sb.Merkle.verify(tree.root(), i, path, leaves[i])
    F = sb.BaseField.main()
    t = g["bfe_tree"]
    tree = sb.Merkle([F(oracle.felt(SEED + t["seed_offset"], i)) for i in range(t["n"])])
    assert tree.root().hex() == t["root"] and [x.hex() for x in tree.nodes] == t["nodes"]


def test_merkle_generic_leaves_like_reference_test(sb):
    """test_merkle.py:58-100 restated: arbitrary picklable leaves, positive and negative openings."""
    from conftest import load_golden as lg
    g = lg("merkle.json")["generic_tree"]
    M64 = (1 << 64) - 1

    def splitmix(x):
        x = (x + 0x9E3779B97F4A7C15) & M64
        z = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)
    leaves = [[bytes((splitmix(i * 1000 + j) & 0xFF) for j in range(splitmix(i) % 200)),
               bytes((splitmix(i * 2000 + j) & 0xFF) for j in range(splitmix(i + 64) % 200))] for i in range(16)]
    tree = sb.Merkle(leaves)
    assert tree.root().hex() == g["root"] and [x.hex() for x in tree.open(5)] == g["path_5"]
    n = 64
    elements = [[os.urandom(os.urandom(1)[0]), os.urandom(os.urandom(1)[0])] for _ in range(n)]
    tree = sb.Merkle(elements)
    root = tree.root()
    for i in range(n):
        path = tree.open(i)
        assert sb.Merkle.verify(root, i, path, elements[i])
        assert not sb.Merkle.verify(root, i, path, os.urandom(51))
        j = (i + 1 + os.urandom(1)[0] % (n - 1)) % n
        assert not sb.Merkle.verify(root, i, path, elements[j])
        assert not sb.Merkle.verify(root, j, path, elements[i])
        assert not sb.Merkle.verify(os.urandom(32), i, path, elements[i])
        for k in range(len(path)):
            assert not sb.Merkle.verify(root, i, path[:k] + [os.urandom(32)] + path[k + 1:], elements[i])


def test_salted_merkle(sb, oracle, monkeypatch):
    g = load_golden("merkle.json")["salted_tree"]
    from stark_brainfuck_amd import salted_merkle
    ctr = [0]

    def fake_urandom(k):
        ctr[0] += 1
        return hashlib.shake_256(b"salt" + ctr[0].to_bytes(8, "little")).digest(k)
    monkeypatch.setattr(salted_merkle, "urandom", fake_urandom)
    XF = sb.ExtensionField.main()
    leaves = [XF.from_limbs([oracle.felt(SEED + g["seed_offset"], 3 * i + k) for k in range(3)]) for i in range(g["n"])]
    tree = sb.SaltedMerkle(leaves)
    assert [l[1].hex() for l in tree.leafs] == g["salts"]
    assert tree.root().hex() == g["root"] and [x.hex() for x in tree.nodes] == g["nodes"]
    salt, path = tree.open(3)
    assert salt.hex() == g["open3_salt"] and [x.hex() for x in path] == g["open3_path"]
    assert sb.SaltedMerkle.verify(tree.root(), 3, salt, path, leaves[3])
    assert not sb.SaltedMerkle.verify(tree.root(), 3, os.urandom(24), path, leaves[3])
    assert not sb.SaltedMerkle.verify(tree.root(), 2, salt, path, leaves[3])


def test_merkle_large_vs_oracle(sb, oracle):
    n = 1 << 12
    soa = oracle.felt_array(SEED + 5, 0, 3 * n).reshape(3, n)
    soa[:, 17] = 0                       # zero element (different pickle template)
    soa[1:, 18] = 0                      # base-field-like element (one stored coefficient)
    soa[2, 19] = 0
    soa[0, 20] = 3                       # short integer opcodes
    tree = sb.Merkle(sb.XArray.from_numpy(soa))
    ref, _ = oracle.xfe_merkle(soa)
    assert tree.root() == ref.root()
    assert tree.nodes[1:] == ref.nodes[1:]
    assert tree.open(1234) == ref.open(1234)


# ------------------------------------------------------------------------------------------------ FRI
def _codeword(sb, oracle, rec, tag):
    d = 1 << rec["log_degree"]
    if tag.startswith("test_fri"):
        coeffs = np.zeros((3, d), dtype=np.uint64)
        coeffs[0] = np.arange(d, dtype=np.uint64)
    else:
        coeffs = oracle.felt_array(SEED, 0, 3 * d).reshape(d, 3).T.copy()
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    fri = sb.Fri(BF.generator(), BF.primitive_nth_root(rec["N"]), rec["N"], rec["expansion"], rec["num_colinearity_tests"], XF)
    assert (fri.domain.offset.value, fri.domain.omega.value) == (rec["offset"], rec["omega"])
    cw = fri.domain.xevaluate(sb.XArray.from_numpy(coeffs), as_array=True)
    soa = cw.to_numpy()
    if rec.get("disturb"):
        for i in rec["disturb"]:
            soa[:, i] = 0
        cw = sb.XArray.from_numpy(soa)
    assert sha_u64(soa) == rec["codeword_sha"]
    return fri, cw, soa, XF


@pytest.mark.parametrize("tag", ["d16_t2", "d64_t8", "d1024_t4", "test_fri_valid", "test_fri_disturbed", "d16_t2_prepushed"])
def test_fri_prove_goldens(sb, oracle, tag):
    rec = load_golden("fri.json")[tag]
    fri, cw, soa, XF = _codeword(sb, oracle, rec, tag)
    ps = sb.ProofStream()
    if rec["num_prepushed"]:
        r = [hashlib.blake2b(bytes([i])).digest() for i in range(2)]
        e = [XF.from_limbs([oracle.felt(SEED + 88, 3 * i + k) for k in range(3)]) for i in range(3)]
        for ob in [r[0], (e[0], e[1], e[2]), [r[1]]]:
            ps.push(ob)
    npre = rec["num_prepushed"]
    root0 = sb.Merkle(cw).root()
    assert root0.hex() == rec["roots"][0]
    idx = fri.prove(cw, ps)
    assert idx == rec["indices"]
    assert len(ps.objects) == rec["num_objects"]
    assert [x.hex() for x in ps.objects[npre:npre + rec["rounds"] - 1]] == rec["roots"][1:]
    assert [[c.value for c in el.polynomial.coefficients] for el in ps.objects[npre + rec["rounds"] - 1]] == rec["last_codeword"]
    ser = ps.serialize()
    assert hashlib.sha256(ser).hexdigest() == rec["serialize_sha256"]
    assert ser == golden_bytes("fri_%s_stream.bin" % tag)
    assert ps.prover_fiat_shamir().hex() == rec["final_fiat_shamir"]
    vs = sb.ProofStream()
    vs.objects, vs.read_index = list(ps.objects), npre
    assert fri.verify(vs, root0) == rec["verify"]


def test_fri_commit_codewords_and_trees(sb, oracle):
    rec = load_golden("fri.json")["d64_t8"]
    fri, cw, soa, XF = _codeword(sb, oracle, rec, "d64_t8")
    ps = sb.ProofStream()
    codewords, trees = fri.commit(cw, ps)
    assert len(codewords) == rec["rounds"] and len(trees) == rec["rounds"] - 1
    assert [sha_u64(c.array.to_numpy()) for c in codewords] == rec["codeword_shas"]
    assert [t.root().hex() for t in trees] == rec["roots"][:-1]
    # fold kernel on its own (bfs_xfe_fold) against the oracle's restatement of fri.py:127-128
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer, synchronize
    out = DeviceBuffer(3 * (rec["N"] // 2))
    alpha = rec["alphas"][0]
    _lib.check(_lib.load().bfs_xfe_fold(cw.ptr, cw.stride, out.ptr, rec["N"] // 2, rec["N"].bit_length() - 1,
                                        (ctypes.c_uint64 * 3)(*alpha), rec["offset"], rec["omega"], 0))
    synchronize(0)
    assert (out.to_numpy().reshape(3, -1) == oracle.fri_fold(soa, alpha, rec["offset"], rec["omega"])).all()
    # Fri.query / query_last on the HBM-resident trees reproduce the transcript prove() writes
    ps2 = sb.ProofStream()
    ps2.objects = list(ps.objects)
    top = fri.sample_indices(ps2.prover_fiat_shamir(), len(codewords[1]), len(codewords[-1]), fri.num_colinearity_tests)
    assert top == rec["indices"]
    indices = list(top)
    for i in range(len(trees) - 1):
        indices = [x % (len(codewords[i]) // 2) for x in indices]
        fri.query(trees[i], trees[i + 1], indices, ps2)
    indices = [x % len(codewords[-1]) for x in indices]
    fri.query_last(trees[-1], codewords[-1], indices, ps2)
    assert len(ps2.objects) == rec["num_objects"]
    assert hashlib.sha256(ps2.serialize()).hexdigest() == rec["serialize_sha256"]


def test_fri_vs_oracle_mid_size(sb, oracle):
    """N = 2^14 (oracle finishes in seconds): every round root, alpha-dependent codeword and the full transcript."""
    log_d, expansion, t = 12, 4, 4
    d, N = 1 << log_d, (1 << log_d) * 4
    coeffs = oracle.felt_array(SEED + 3, 0, 3 * d).reshape(d, 3).T.copy()
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    fri = sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, expansion, t, XF)
    cw = fri.domain.xevaluate(sb.XArray.from_numpy(coeffs), as_array=True)
    soa = cw.to_numpy()
    ref = oracle.fri_prove(soa, 7, oracle.primitive_nth_root(N), expansion, t)
    ps = sb.ProofStream()
    assert fri.prove(cw, ps) == ref["indices"]
    assert ps.serialize() == ref["proof_stream"].serialize()


def test_config3_fri_2p20(sb, oracle):
    """BASELINE config 3: FRI.prove on a degree-2^18 codeword, expansion 4.  Against the reference's own run when its
    fixture exists (fri20.json), and always through verify() and the round-0 root."""
    log_d, expansion, t = 18, 4, 4
    d, N = 1 << log_d, (1 << log_d) * 4
    coeffs = oracle.felt_array(SEED, 0, 3 * d).reshape(d, 3).T.copy()
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    fri = sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, expansion, t, XF)
    cw = fri.domain.xevaluate(sb.XArray.from_numpy(coeffs), as_array=True)
    root0 = sb.Merkle(cw).root()
    ps = sb.ProofStream()
    idx = fri.prove(cw, ps)
    assert len(set(i % 8 for i in idx)) == t and all(0 <= i < N // 2 for i in idx)
    vs = sb.ProofStream()
    vs.objects = list(ps.objects)
    assert fri.verify(vs, root0)
    bad = sb.ProofStream()
    bad.objects = list(ps.objects)
    bad.objects[0] = bytes(64)           # a wrong round-1 root changes every later challenge
    assert not fri.verify(bad, root0)
    path = os.path.join(GOLDEN, "fri20.json")
    if os.path.exists(path):
        rec = load_golden("fri20.json")
        assert sha_u64(cw.to_numpy()) == rec["codeword_sha"]
        assert root0.hex() == rec["roots"][0]
        assert [x.hex() for x in ps.objects[:rec["rounds"] - 1]] == rec["roots"][1:]
        assert idx == rec["indices"] and len(ps.objects) == rec["num_objects"]
        ser = ps.serialize()
        assert (len(ser), hashlib.sha256(ser).hexdigest()) == (rec["serialize_len"], rec["serialize_sha256"])


def test_fri_length_assert(sb):
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    fri = sb.Fri(BF.generator(), BF.primitive_nth_root(64), 64, 4, 2, XF)
    with pytest.raises(AssertionError) as e:
        fri.prove([XF.zero()] * 32, sb.ProofStream())
    assert str(e.value) == load_golden("fri.json")["errors"]["length_mismatch"]


def test_smoke_entry_point(sb):
    import __graft_entry__
    __graft_entry__.smoke()


# ------------------------------------------------------------------------------------------------ plumbing entry points
def test_field_primitives_device_vs_host(sb):
    """every field primitive and a set of compositions (with compile-time constants) must give the same result on the
    device as the plain 128-bit host arithmetic: guards against compiler folds across the carry chains (gl.hpp, gl_sub)"""
    from stark_brainfuck_amd import _lib
    lib = _lib.load()
    bad = ctypes.c_uint64(1)
    _lib.check(lib.bfs_selftest_field(18, ctypes.byref(bad)))
    assert bad.value == 0, lib.bfs_last_error().decode()


def test_c_abi_plumbing_and_elementwise(sb, oracle):
    """bfs_gl_scale / bfs_gl_mul_pointwise / bfs_gl_batch_inverse / memcpy_d2d / memset / events, straight through the C ABI."""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer, synchronize
    lib = _lib.load()
    n = 5000                                   # not a power of two on purpose
    a, b = oracle.felt_array(SEED + 1, 0, n), oracle.felt_array(SEED + 2, 0, n)
    da, db, dc = DeviceBuffer.from_numpy(a), DeviceBuffer.from_numpy(b), DeviceBuffer(n)
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(lib.bfs_event_create(ctypes.byref(e0))); _lib.check(lib.bfs_event_create(ctypes.byref(e1)))
    _lib.check(lib.bfs_event_record(e0, 0))
    _lib.check(lib.bfs_gl_mul_pointwise(da.ptr, db.ptr, dc.ptr, n, 0))
    _lib.check(lib.bfs_event_record(e1, 0))
    ms = ctypes.c_float()
    _lib.check(lib.bfs_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
    assert ms.value >= 0
    assert (dc.to_numpy() == oracle.hadamard(a, b)).all()
    _lib.check(lib.bfs_gl_scale(da.ptr, dc.ptr, n, n, 1, 7, 0))
    assert (dc.to_numpy() == oracle.scale(7, a)).all()
    a1 = np.where(a == 0, np.uint64(1), a)
    da1 = DeviceBuffer.from_numpy(a1)
    _lib.check(lib.bfs_gl_batch_inverse(da1.ptr, dc.ptr, n, 0))
    assert (dc.to_numpy() == oracle.batch_inverse(a1)).all()
    a1[17] = 0
    with pytest.raises(AssertionError, match="batch inverse does not work when input contains a zero"):
        _lib.check(lib.bfs_gl_batch_inverse(DeviceBuffer.from_numpy(a1).ptr, dc.ptr, n, 0))
    _lib.check(lib.bfs_memcpy_d2d(dc.ptr, db.ptr, n * 8, 0))
    assert (dc.to_numpy() == b).all()
    _lib.check(lib.bfs_memset(dc.ptr, 0, n * 8, 0))
    synchronize(0)
    assert not dc.to_numpy().any()
    cnt = ctypes.c_int()
    _lib.check(lib.bfs_device_count(ctypes.byref(cnt)))
    assert cnt.value >= 1
    lib.bfs_event_destroy(e0); lib.bfs_event_destroy(e1)
    # HBM-resident arrays through the mirror: nothing is copied to the host
    F = sb.BaseField.main()
    arr = sb.BaseArray.from_numpy(oracle.felt_array(SEED, 0, 1 << 12))
    w = F.primitive_nth_root(1 << 12)
    out = sb.ntt(w, arr)
    assert isinstance(out, sb.BaseArray) and (sb.intt(w, out).to_numpy() == arr.to_numpy()).all()
    inv = sb.batch_inverse(sb.BaseArray.from_numpy(a1 + np.uint64(a1[17] == 0)))
    assert isinstance(inv, sb.BaseArray)


def test_salted_merkle_over_zipped_tuples(sb, oracle, monkeypatch):
    """leaf = tuple of one extension and several base elements, as BrainfuckStark zips its codewords
    (brainfuck_stark.py:178-180); preimages come from the native emitter, hashing from the GPU; checked against the oracle."""
    from stark_brainfuck_amd import salted_merkle
    ctr = [0]

    def fake_urandom(k):
        ctr[0] += 1
        return hashlib.shake_256(b"zip" + ctr[0].to_bytes(8, "little")).digest(k)
    monkeypatch.setattr(salted_merkle, "urandom", fake_urandom)
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    n, cols = 16, 5
    leaves, oleaves = [], []
    for i in range(n):
        x = [oracle.felt(SEED + 31, 3 * i + k) for k in range(3)]
        bs = [oracle.felt(SEED + 32 + j, i) for j in range(cols)]
        leaves.append(tuple([XF.from_limbs(x)] + [sb.BaseFieldElement(v, BF) for v in bs]))
        oleaves.append(tuple([oracle.make_xfe(x)] + [oracle.make_bfe(v, internal=True) for v in bs]))
    tree = sb.SaltedMerkle(leaves)
    salts = [hashlib.shake_256(b"zip" + (i + 1).to_bytes(8, "little")).digest(24) for i in range(n)]
    ref = oracle.MerkleOracle([oracle.salted_leaf_bytes(l, s) for l, s in zip(oleaves, salts)])
    assert tree.root() == ref.root()
    salt, path = tree.open(5)
    assert salt == salts[5] and path == ref.open(5)
    assert sb.SaltedMerkle.verify(tree.root(), 5, salt, path, leaves[5])


def test_zipped_rows_commitment_on_device_vs_oracle(sb, oracle, monkeypatch):
    """bfs_merkle_build_rows (csrc/rows.hip): every row's pickle is synthesised on the GPU from a per-pattern template.
    Rows here mix all coefficient counts (0..3 stored coefficients per extension element, so memo indices shift from row
    to row) and all integer opcode widths (BININT1 / BININT2 / BININT / LONG1 of 5..9 bytes); the oracle pickles every
    row with CPython on look-alike classes, exactly like brainfuck_stark.py:178-179 + salted_merkle.py:32-35."""
    from stark_brainfuck_amd import salted_merkle
    from stark_brainfuck_amd.device import DeviceBuffer
    from stark_brainfuck_amd.salted_merkle import ZippedSaltedMerkle
    P = (1 << 64) - (1 << 32) + 1
    n = 1 << 9
    rng = np.random.default_rng(0xB0B)
    edges = [0, 1, 255, 256, 65535, 65536, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 39, (1 << 47) - 1, 1 << 47, (1 << 55), (1 << 63) - 1, 1 << 63, P - 1]

    def column(kind):
        vals = rng.integers(0, P, n, dtype=np.uint64)
        pick = rng.integers(0, 4, n)
        vals = np.where(pick == 0, np.array([edges[i % len(edges)] for i in range(n)], dtype=np.uint64), vals)
        if kind == "zero":
            vals[:] = 0
        elif kind == "sparse":
            vals[rng.integers(0, 2, n) == 0] = 0
        return vals
    # 3 extension columns (limb planes with different zero patterns -> k = 0..3) and 5 base columns
    ext = [np.stack([column("any"), column("sparse"), column("sparse")]), np.stack([column("sparse"), column("zero"), column("zero")]),
           np.stack([column("sparse"), column("sparse"), column("zero")])]
    base = [column("any") for _ in range(5)]
    order = ["x0", "b0", "b1", "x1", "b2", "x2", "b3", "b4"]          # extension and base columns interleaved
    bufs, cols = [], []
    for name in order:
        data = ext[int(name[1])] if name[0] == "x" else base[int(name[1])]
        buf = DeviceBuffer.from_numpy(np.ascontiguousarray(data).reshape(-1))
        bufs.append(buf)
        cols.append((buf.ptr, name[0] == "x", 0))
    salts = rng.integers(0, 256, 24 * n, dtype=np.uint8).tobytes()
    monkeypatch.setattr(salted_merkle, "urandom", lambda count: salts[:count])
    tree = ZippedSaltedMerkle(cols, n, lambda i: None)

    def orow(i):
        items = []
        for name in order:
            if name[0] == "x":
                e = ext[int(name[1])]
                items.append(oracle.make_xfe([int(e[0, i]), int(e[1, i]), int(e[2, i])]))
            else:
                items.append(oracle.make_bfe(int(base[int(name[1])][i])))
        return tuple(items)
    ref = oracle.MerkleOracle([oracle.salted_leaf_bytes(orow(i), salts[24 * i:24 * i + 24]) for i in range(n)])
    patterns = {tuple(len(oracle.xtrim([int(e[0, i]), int(e[1, i]), int(e[2, i])])) for e in ext) for i in range(n)}
    assert len(patterns) >= 8, "the test data should exercise many coefficient-count patterns"
    assert tree.root() == ref.root()
    assert tree.open(5)[1] == ref.open(5)
    # unsalted rows go through the same kernel (no second pickle)
    from stark_brainfuck_amd import _lib
    lib = _lib.load()
    nodes = DeviceBuffer(2 * n * 8)
    rc = (_lib.RowColumn * len(cols))()
    for r, (ptr, is_ext, fid) in zip(rc, cols):
        r.d_values, r.is_ext, r.field_id = ptr, int(is_ext), fid
    _lib.check(lib.bfs_merkle_build_rows(rc, len(cols), n, None, 0, nodes.ptr, 0))
    ref2 = oracle.MerkleOracle([oracle.dumps(orow(i)) for i in range(n)])
    assert nodes.to_numpy(8, offset=8).tobytes() == ref2.root()
    # salts expanded on the device (bfs_random_fill): the tree must be the tree of exactly those salts
    monkeypatch.undo()
    tree3 = ZippedSaltedMerkle(cols, n, lambda i: None)
    dsalts = tree3._salts.to_numpy(3 * n).tobytes()
    assert len(set(dsalts[24 * i:24 * i + 24] for i in range(n))) == n
    ref3 = oracle.MerkleOracle([oracle.salted_leaf_bytes(orow(i), dsalts[24 * i:24 * i + 24]) for i in range(n)])
    assert tree3.root() == ref3.root()
    assert tree3.leafs[7][1] == dsalts[24 * 7:24 * 8]
    import hashlib
    seed = bytes(range(32))
    buf = DeviceBuffer(16)
    _lib.check(lib.bfs_random_fill(seed, buf.ptr, 16, 0))
    got = buf.to_numpy(16).tobytes()
    assert got[:64] == hashlib.blake2b(seed + (0).to_bytes(8, "little")).digest()
    assert got[64:] == hashlib.blake2b(seed + (1).to_bytes(8, "little")).digest()


def test_ntt_batch_larger_than_grid_limit(sb, oracle):
    """more than 65535 independent transforms in one call (the batch index lives in grid.y): sliced internally"""
    logn, batch = 5, 70001
    n = 1 << logn
    rng = np.random.default_rng(5)
    v = rng.integers(0, (1 << 64) - (1 << 32) + 1, n * batch, dtype=np.uint64)
    w = oracle.primitive_nth_root(n)
    out = raw_ntt(sb, v, logn, w, batch=batch).reshape(batch, n)
    for b in (0, 1, 65534, 65535, 65536, batch - 1):
        assert (out[b] == oracle.ntt(w, v[b * n:(b + 1) * n])).all(), b
    lo = raw_ntt(sb, v[:n * 40000], logn, w, batch=40000).reshape(40000, n)
    hi = raw_ntt(sb, v[n * 40000:], logn, w, batch=batch - 40000).reshape(batch - 40000, n)
    assert (out[:40000] == lo).all() and (out[40000:] == hi).all()


def test_device_side_sampling_of_the_randomizer_polynomial(sb):
    """bfs_xfe_sample_fill: ExtensionField.sample (extension_field.py:100-111) of 27 pseudo-random bytes per element; the byte stream
    is the first 63 bytes of every BLAKE2b-512(seed || block counter), element i takes bytes [27 i, 27 i + 27)"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer
    lib = _lib.load()
    P = (1 << 64) - (1 << 32) + 1
    seed = bytes(range(100, 132))
    for count in (1, 2, 3, 7, 1000, 4099):
        buf = DeviceBuffer(3 * count)
        _lib.check(lib.bfs_xfe_sample_fill(seed, buf.ptr, count, count, 0))
        got = buf.to_numpy(3 * count).reshape(3, count)
        blocks = (27 * count + 62) // 63
        stream = b"".join(hashlib.blake2b(seed + b.to_bytes(8, "little")).digest()[:63] for b in range(blocks))
        for i in sorted({0, 1, 2, count // 2, count - 1}):
            if i >= count:
                continue
            chunk = stream[27 * i:27 * i + 27]
            for j in range(3):
                assert int(got[j, i]) == int.from_bytes(chunk[9 * j:9 * j + 9], "big") % P, (count, i, j)
        assert (got < np.uint64(P)).all()
        if count >= 1000:
            assert len(set(got.reshape(-1).tolist())) == 3 * count


def test_zipped_rows_remembered_patterns_and_the_fallback(sb, oracle):
    """bfs_merkle_build_rows tries the row patterns its column layout had LAST time before collecting them (no pattern kernel, no
    read-back in the middle of the call) and hashes again when a row turns up without a template: three commitments of one layout --
    all elements of full degree, then rows with zero and short elements (new patterns: the fallback), then full degree again (the
    remembered set is now a superset) -- each against the oracle's pickles"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer
    lib = _lib.load()
    P = (1 << 64) - (1 << 32) + 1
    n = 1 << 10
    rng = np.random.default_rng(0xFA11)

    def commit(ext, base):
        bufs = [DeviceBuffer.from_numpy(np.ascontiguousarray(e).reshape(-1)) for e in ext] + [DeviceBuffer.from_numpy(b) for b in base]
        rc = (_lib.RowColumn * len(bufs))()
        for r, b, is_ext in zip(rc, bufs, [1] * len(ext) + [0] * len(base)):
            r.d_values, r.is_ext, r.field_id = b.ptr, is_ext, 0
        nodes = DeviceBuffer(2 * n * 8)
        _lib.check(lib.bfs_merkle_build_rows(rc, len(bufs), n, None, 0, nodes.ptr, 0))
        rows = [tuple([oracle.make_xfe([int(e[0, i]), int(e[1, i]), int(e[2, i])]) for e in ext] + [oracle.make_bfe(int(b[i])) for b in base]) for i in range(n)]
        assert nodes.to_numpy(8, offset=8).tobytes() == oracle.MerkleOracle([oracle.dumps(r) for r in rows]).root()
    full = lambda: rng.integers(1 << 40, P, (3, n), dtype=np.uint64)
    base = [rng.integers(0, P, n, dtype=np.uint64) for _ in range(2)]
    commit([full(), full()], base)
    holes = full()
    holes[:, 5] = 0                       # a zero element
    holes[2, 100:140] = 0                 # two stored coefficients
    holes[1:, 700] = 0                    # one
    commit([full(), holes], base)
    commit([full(), full()], base)
    commit([holes, holes], base)


@pytest.mark.parametrize("n,n_ext,n_base", [(1, 1, 0), (2, 0, 3), (3, 2, 2), (65, 16, 16), (1000, 2, 2)])
def test_zipped_rows_edge_shapes(sb, oracle, n, n_ext, n_base):
    """row emitter on tiny, ragged (absent leaf slots) and wide inputs; 32 columns make the row pickle longer than 2.5 KB,
    with memo back-references beyond index 255 (LONG_BINGET); the zeroed limbs put several patterns into one wave, so
    the leaf kernel walks several templates per wave (lanes of another template wait their turn); the base columns hold
    one-byte integers next to the 9-byte ones of the extension limbs, and the extension rows alternate between
    coefficient counts, so the lanes of a wave drift apart in their block buffers"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer
    lib = _lib.load()
    P = (1 << 64) - (1 << 32) + 1
    rng = np.random.default_rng(n * 100 + n_ext)
    ext = [rng.integers(0, P, (3, n), dtype=np.uint64) for _ in range(n_ext)]
    for e in ext:
        e[2, ::2] = 0
        e[1, ::4] = 0
        e[0, ::8] = 0
    base = [rng.integers(0, 300, n, dtype=np.uint64) for _ in range(n_base)]
    bufs = [DeviceBuffer.from_numpy(np.ascontiguousarray(e).reshape(-1)) for e in ext] + [DeviceBuffer.from_numpy(b) for b in base]
    rc = (_lib.RowColumn * len(bufs))()
    for k, b in enumerate(bufs):
        rc[k].d_values, rc[k].is_ext, rc[k].field_id = b.ptr, int(k < n_ext), 0
    npo2 = 1
    while npo2 < n:
        npo2 <<= 1
    nodes = DeviceBuffer(2 * npo2 * 8)
    salts = rng.integers(0, 256, 24 * n, dtype=np.uint8).tobytes()
    keep = ctypes.create_string_buffer(salts, len(salts))
    _lib.check(lib.bfs_merkle_build_rows(rc, len(bufs), n, ctypes.cast(keep, ctypes.c_void_p), 0, nodes.ptr, 0))
    rows = [tuple([oracle.make_xfe([int(e[0, i]), int(e[1, i]), int(e[2, i])]) for e in ext] + [oracle.make_bfe(int(b[i])) for b in base])
            for i in range(n)]
    ref = oracle.MerkleOracle([oracle.salted_leaf_bytes(r, salts[24 * i:24 * i + 24]) for i, r in enumerate(rows)])
    assert nodes.to_numpy(8, offset=8).tobytes() == ref.root()


@pytest.mark.gpu
@pytest.mark.parametrize("n_ext,n_base", [(1, 16), (9, 0)])
def test_zipped_rows_generated_layouts(sb, oracle, n_ext, n_base):
    """the prover's two column layouts go through the straight-line kernels of csrc/rows_generated.hpp (tools/gen_rows.py): every
    leaf digest against the oracle's pickles, for (a) rows of random field elements, (b) rows whose integers have every opcode width
    -- one-byte values next to nine-byte ones, so the lanes of a wave drift whole blocks apart -- but whose extension elements still
    store three coefficients, (c) the same with some top limbs zero: those rows are another pattern, the generated kernel leaves
    them to the interpreter kernel launched behind it (first through the fallback of a remembered pattern set that lacks them),
    (d) a layout one column wider, which must NOT take a generated kernel."""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer
    lib = _lib.load()
    P = (1 << 64) - (1 << 32) + 1
    n, npo2 = 1000, 1024
    rng = np.random.default_rng(900 + n_ext)
    widths = [1, 200, 60000, (1 << 31) - 1, 1 << 31, (1 << 40) + 5, (1 << 48) - 1, 1 << 55, (1 << 56) - 1, 1 << 56, (1 << 63) - 1, 1 << 63, P - 1]

    def commit(ext, base, expect_generated):
        bufs = [DeviceBuffer.from_numpy(np.ascontiguousarray(e).reshape(-1)) for e in ext] + [DeviceBuffer.from_numpy(np.ascontiguousarray(b)) for b in base]
        rc = (_lib.RowColumn * len(bufs))()
        for k, b in enumerate(bufs):
            rc[k].d_values, rc[k].is_ext, rc[k].field_id = b.ptr, int(k < len(ext)), 0
        nodes = DeviceBuffer(2 * npo2 * 8)
        salts = rng.integers(0, 256, 24 * n, dtype=np.uint8).tobytes()
        keep = ctypes.create_string_buffer(salts, len(salts))
        before = lib.bfs_row_generated_launches()
        _lib.check(lib.bfs_merkle_build_rows(rc, len(bufs), n, ctypes.cast(keep, ctypes.c_void_p), 0, nodes.ptr, 0))
        assert (lib.bfs_row_generated_launches() > before) == expect_generated
        rows = [tuple([oracle.make_xfe([int(e[0, i]), int(e[1, i]), int(e[2, i])]) for e in ext] + [oracle.make_bfe(int(b[i])) for b in base])
                for i in range(n)]
        pre = [oracle.salted_leaf_bytes(r, salts[24 * i:24 * i + 24]) for i, r in enumerate(rows)]
        got = nodes.to_numpy(8 * n, offset=8 * npo2).tobytes()
        bad = [i for i in range(n) if got[64 * i:64 * i + 64] != hashlib.blake2b(pre[i]).digest()]
        assert not bad, "leaf digests differ at rows %s" % bad[:8]
        assert nodes.to_numpy(8, offset=8).tobytes() == oracle.MerkleOracle(pre).root()
        return pre

    # (a) random field elements; for the extension commitment also the patterns of its last two columns the header has variants for
    # (the evaluation columns of the input and output tables: zero without symbols, a base-field constant with one)
    ext = [rng.integers(1, P, (3, n), dtype=np.uint64) for _ in range(n_ext)]
    base = [rng.integers(0, P, n, dtype=np.uint64) for _ in range(n_base)]
    commit(ext, base, True)
    if n_ext == 9:
        for k7, k8 in [(0, 3), (0, 1), (1, 0), (3, 1), (0, 0), (1, 1)]:
            e = [x.copy() for x in ext]
            e[7][k7:] = 0
            e[8][k8:] = 0
            commit(e, base, True)
            commit(e, base, True)             # (the second time through the remembered pattern set)
        e = [x.copy() for x in ext]
        e[7][2:] = 0                          # two stored coefficients: no variant for that ...
        commit(e, base, True)                 # ... (found out by the generated kernel the remembered pattern set stood for) ...
        commit(e, base, False)                # ... so the interpreter alone
        commit(ext, base, True)
    # (b) every opcode width, neighbouring rows far apart; top limbs stay non-zero
    ext = [np.zeros((3, n), dtype=np.uint64) for _ in range(n_ext)]
    base = [np.zeros(n, dtype=np.uint64) for _ in range(n_base)]
    for i in range(n):
        kind = i % 4
        for c, col in enumerate([e[j] for e in ext for j in range(3)] + base):
            if kind == 0:
                col[i] = 7
            elif kind == 1:
                col[i] = P - 1 - c
            elif kind == 2:
                col[i] = widths[(i + c) % len(widths)]
            else:
                col[i] = widths[int(rng.integers(0, len(widths)))] if c < (i % 27) else 3
    pre = commit(ext, base, True)
    lengths = {len(p) for p in pre}
    assert max(lengths) - min(lengths) >= 9 * (3 * n_ext + n_base) - 20
    # (c) rows of other patterns among them: a zero element, two stored coefficients, one
    for e in ext[:2]:
        e[:, 5] = 0
        e[2, 100:140] = 0
        e[1:, 700] = 0
    ext[-1][2, 256:512] = 0               # a whole workgroup of the generated kernel with nothing to do
    commit(ext, base, True)               # (remembered set: one pattern; rows without a template -> collected, hashed again)
    commit(ext, base, True)               # (remembered set: all of them; generated kernel + interpreter, no fallback)
    # (d) one base column more: not a layout the header knows
    commit(ext, base + [rng.integers(0, P, n, dtype=np.uint64)], False)


@pytest.mark.gpu
@pytest.mark.parametrize("salted", [True, False])
def test_zipped_rows_lanes_far_apart(sb, oracle, salted):
    """the leaf kernel compresses wave-synchronously: every lane has a 24-word block buffer and the wave compresses when the lane
    furthest ahead has filled it.  Here neighbouring rows differ by up to 32 x 9 = 288 bytes of preimage (all integers one byte
    long in one row, nine bytes in the next, mixed widths in others), so lanes are whole blocks apart, sit compressions out, and
    finish with different numbers of blocks.  Every leaf digest is compared, not only the root."""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer
    lib = _lib.load()
    P = (1 << 64) - (1 << 32) + 1
    n, n_base = 333, 32
    rng = np.random.default_rng(7)
    widths = [0, 200, 60000, (1 << 31) - 1, 1 << 31, (1 << 40) + 5, (1 << 48) - 1, 1 << 55, (1 << 63) - 1, P - 1]
    base = np.zeros((n_base, n), dtype=np.uint64)
    for i in range(n):
        kind = i % 4
        for c in range(n_base):
            if kind == 0:
                base[c, i] = 7                                      # two bytes each
            elif kind == 1:
                base[c, i] = P - 1 - c                              # eleven bytes each
            elif kind == 2:
                base[c, i] = widths[(i + c) % len(widths)]
            else:
                base[c, i] = widths[int(rng.integers(0, len(widths)))] if c < (i % n_base) else 3
    bufs = [DeviceBuffer.from_numpy(np.ascontiguousarray(base[c])) for c in range(n_base)]
    rc = (_lib.RowColumn * n_base)()
    for k, b in enumerate(bufs):
        rc[k].d_values, rc[k].is_ext, rc[k].field_id = b.ptr, 0, 0
    npo2 = 512
    nodes = DeviceBuffer(2 * npo2 * 8)
    salts = rng.integers(0, 256, 24 * n, dtype=np.uint8).tobytes()
    keep = ctypes.create_string_buffer(salts, len(salts))
    _lib.check(lib.bfs_merkle_build_rows(rc, n_base, n, ctypes.cast(keep, ctypes.c_void_p) if salted else None, 0, nodes.ptr, 0))
    rows = [tuple(oracle.make_bfe(int(base[c, i])) for c in range(n_base)) for i in range(n)]
    preimages = [oracle.salted_leaf_bytes(r, salts[24 * i:24 * i + 24]) if salted else oracle.dumps(r) for i, r in enumerate(rows)]
    lengths = {len(p) for p in preimages}
    assert max(lengths) - min(lengths) >= 280, "the rows should differ by more than two blocks of preimage"
    ref = oracle.MerkleOracle(preimages)
    got = nodes.to_numpy(8 * n, offset=8 * npo2).tobytes()
    for i in range(n):
        assert got[64 * i:64 * i + 64] == hashlib.blake2b(preimages[i]).digest(), "leaf %d (%d bytes)" % (i, len(preimages[i]))
    assert nodes.to_numpy(8, offset=8).tobytes() == ref.root()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 255, 256, 257, 4099, 70001, (1 << 17) + 3])
def test_device_scan_matches_the_host_scan(sb, n):
    """bfs_xfe_scan_device (prefix scan of affine maps, csrc/scan.hip) against the sequential host primitive bfs_xfe_scan on the
    same columns: both kinds, masks present and absent, recording before / after the update, a shifted first column"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer, current_stream
    from stark_brainfuck_amd.table import Table
    lib, stream = _lib.load(), current_stream()
    P = (1 << 64) - (1 << 32) + 1
    rng = np.random.default_rng(n)
    cols = rng.integers(0, P, (3, n), dtype=np.uint64)
    cols[1, rng.integers(0, n, max(1, n // 7))] = 0
    d_cols = DeviceBuffer.from_numpy(cols.reshape(-1))
    mask = rng.integers(0, 4, n) != 0
    d_mask = DeviceBuffer((n + 7) // 8)
    m8 = np.ascontiguousarray(mask, dtype=np.uint8)
    _lib.check(lib.bfs_memcpy_h2d(d_mask.ptr, m8.ctypes.data, n, stream))
    u64 = ctypes.c_uint64
    for kind, ncols, use_mask, before, shift1 in [(0, 3, True, True, 0), (0, 3, False, False, 0), (1, 1, True, True, 1),
                                                  (1, 3, True, False, 0), (1, 1, False, False, 0), (0, 2, True, False, 3 % n)]:
        constants = [tuple(int(v) for v in rng.integers(0, P, 3, dtype=np.uint64)) for _ in range(1 + ncols)]
        initial = tuple(int(v) for v in rng.integers(0, P, 3, dtype=np.uint64))
        host_cols = [cols[c] for c in range(ncols)]
        if shift1:
            host_cols[0] = np.roll(host_cols[0], -shift1)
        want, want_terminal = Table.scan(kind, host_cols, mask if use_mask else None, constants, initial, before)
        out, d_terminal = DeviceBuffer(3 * n), DeviceBuffer(3)
        terminal = (u64 * 3)()
        ptrs = [d_cols.ptr + 8 * c * n for c in range(ncols)] + [None] * (3 - ncols)
        flat = [v for c in constants for v in c] + [0] * (12 - 3 * len(constants))
        _lib.check(lib.bfs_xfe_scan_device(kind, ptrs[0], ptrs[1], ptrs[2], shift1, d_mask.ptr if use_mask else None, n,
                                           (u64 * 12)(*flat), (u64 * 3)(*initial), 1 if before else 0, out.ptr, n, d_terminal.ptr, terminal, stream))
        got = out.to_numpy(3 * n).reshape(3, n)
        assert tuple(int(v) for v in terminal) == want_terminal, (kind, ncols, use_mask, before, shift1)
        assert tuple(int(v) for v in d_terminal.to_numpy(3)) == want_terminal
        assert (got == want).all(), (kind, ncols, use_mask, before, shift1)


@pytest.mark.gpu
def test_scans_side_by_side_match_the_host_scan(sb):
    """bfs_xfe_scan_device_many: scans of different kinds, lengths (1 .. 70 000 rows: one workgroup up to the 256-workgroup cap with
    several rows per thread), masks, shifts and recording modes in ONE call (blockIdx.y = scan), each against the sequential host
    primitive; the bad-argument paths"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer, current_stream
    from stark_brainfuck_amd.table import Table
    lib, stream = _lib.load(), current_stream()
    P = (1 << 64) - (1 << 32) + 1
    rng = np.random.default_rng(77)
    u64 = ctypes.c_uint64
    plans = [(0, 3, True, True, 0, 1), (1, 1, False, False, 0, 2), (0, 2, True, False, 3, 255), (1, 3, True, True, 1, 256), (1, 1, True, False, 0, 257),
             (0, 3, False, True, 0, 4096), (0, 1, True, False, 5, 65536), (1, 2, False, False, 0, 70000), (0, 3, True, True, 0, 1000)]
    specs, keep, wants = [], [], []
    for kind, ncols, use_mask, before, shift1, n in plans:
        cols = rng.integers(0, P, (3, n), dtype=np.uint64)
        cols[1, rng.integers(0, n, max(1, n // 7))] = 0
        d_cols = DeviceBuffer.from_numpy(cols.reshape(-1))
        mask = rng.integers(0, 4, n) != 0
        d_mask = DeviceBuffer((n + 7) // 8)
        m8 = np.ascontiguousarray(mask, dtype=np.uint8)
        _lib.check(lib.bfs_memcpy_h2d(d_mask.ptr, m8.ctypes.data, n, stream))
        constants = [tuple(int(v) for v in rng.integers(0, P, 3, dtype=np.uint64)) for _ in range(1 + ncols)]
        initial = tuple(int(v) for v in rng.integers(0, P, 3, dtype=np.uint64))
        host_cols = [cols[c] for c in range(ncols)]
        shift1 %= n
        if shift1:
            host_cols[0] = np.roll(host_cols[0], -shift1)
        wants.append(Table.scan(kind, host_cols, mask if use_mask else None, constants, initial, before))
        out, d_terminal = DeviceBuffer(3 * n), DeviceBuffer(3)
        ptrs = [d_cols.ptr + 8 * c * n for c in range(ncols)] + [None] * (3 - ncols)
        flat = [v for c in constants for v in c] + [0] * (12 - 3 * len(constants))
        specs.append(_lib.ScanSpec(kind, 1 if before else 0, ptrs[0], ptrs[1], ptrs[2], shift1, d_mask.ptr if use_mask else None, n,
                                   (u64 * 12)(*flat), (u64 * 3)(*initial), out.ptr, n, d_terminal.ptr))
        keep.append((d_cols, d_mask, out, d_terminal, n))
    _lib.check(lib.bfs_xfe_scan_device_many((_lib.ScanSpec * len(specs))(*specs), len(specs), stream))
    for plan, (_, _, out, d_terminal, n), (want, want_terminal) in zip(plans, keep, wants):
        assert tuple(int(v) for v in d_terminal.to_numpy(3)) == want_terminal, plan
        assert (out.to_numpy(3 * n).reshape(3, n) == want).all(), plan
    assert lib.bfs_xfe_scan_device_many(None, 0, stream) == 0
    bad = _lib.ScanSpec(2, 0, keep[0][0].ptr, None, None, 0, None, 1, (u64 * 12)(), (u64 * 3)(), keep[0][2].ptr, 1, None)
    assert lib.bfs_xfe_scan_device_many((_lib.ScanSpec * 1)(bad), 1, stream) != 0 and b"kind" in lib.bfs_last_error()
    empty = _lib.ScanSpec(0, 0, keep[0][0].ptr, None, None, 0, None, 0, (u64 * 12)(), (u64 * 3)(), keep[0][2].ptr, 1, None)
    assert lib.bfs_xfe_scan_device_many((_lib.ScanSpec * 1)(empty), 1, stream) != 0
    assert lib.bfs_xfe_scan_device_many((_lib.ScanSpec * 65)(*([specs[0]] * 65)), 65, stream) != 0


@pytest.mark.gpu
def test_memory_pools(sb):
    """bfs_malloc_async / bfs_free_async: a freed block is handed out again without going to the driver, the statistics add up,
    bfs_pool_trim gives the cache back, pinned staging arrays copy correctly, the stream-less pair keeps hipMalloc semantics"""
    from stark_brainfuck_amd import _lib, device
    from stark_brainfuck_amd.device import DeviceBuffer
    lib = _lib.load()
    device.synchronize()
    device.pool_trim()
    live0, cached0 = device.pool_stats()
    assert cached0 == 0
    a = DeviceBuffer(3 << 17)                      # 3 MiB -> a size class of its own
    ptr = a.ptr
    live1, _ = device.pool_stats()
    assert live1 - live0 >= 3 << 20
    a.free()
    live2, cached2 = device.pool_stats()
    assert live2 == live0 and cached2 == live1 - live0
    b = DeviceBuffer(3 << 17)
    assert b.ptr == ptr and device.pool_stats()[1] == 0          # the same block, straight from the free list
    data = np.arange(3 << 17, dtype=np.uint64)
    staged = device.pinned_empty(data.shape)
    staged[:] = data
    _lib.check(lib.bfs_memcpy_h2d(b.ptr, staged.ctypes.data, data.nbytes, device.current_stream()))
    assert (b.to_numpy() == data).all()                          # to_numpy: the staged path for a 3 MiB pageable destination
    c = DeviceBuffer.from_numpy(data[::-1].copy())               # pageable source, staged through the pinned pool
    assert (c.to_numpy() == data[::-1]).all()
    b.free(); c.free()
    assert device.pool_stats()[1] > 0
    device.pool_trim()
    assert device.pool_stats() == (live0, 0)
    p = ctypes.c_void_p()
    _lib.check(lib.bfs_malloc(ctypes.byref(p), 1 << 20))
    _lib.check(lib.bfs_free(p))
    assert lib.bfs_free(ctypes.c_void_p(12345)) != 0 and b"did not allocate" in lib.bfs_last_error()
    device.pool_trim()


@pytest.mark.parametrize("n", [1, 2, 7, 255, 256, 2047, 2048, 2049, 100003, (1 << 20) + 5])
def test_batch_inverse_and_scale_ragged_sizes(sb, oracle, n):
    """bfs_gl_batch_inverse (one inversion per 2048 elements, Montgomery's trick across a workgroup) and bfs_gl_scale (power tables of
    an arbitrary factor built on the device) on sizes that leave threads and workgroups partly empty; in place as well (ntt.py:177-188,
    univariate.py:168-169)"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer, synchronize
    lib = _lib.load()
    P = (1 << 64) - (1 << 32) + 1
    a = oracle.felt_array(SEED + n, 0, n)
    a = np.where(a == 0, np.uint64(1), a)
    a[n // 2] = P - 1
    a[0] = 1
    da, dc = DeviceBuffer.from_numpy(a), DeviceBuffer(n)
    _lib.check(lib.bfs_gl_batch_inverse(da.ptr, dc.ptr, n, 0))
    want = oracle.batch_inverse(a)
    assert (dc.to_numpy() == want).all()
    _lib.check(lib.bfs_gl_batch_inverse(da.ptr, da.ptr, n, 0))          # in place (fast_coset_divide does this)
    assert (da.to_numpy() == want).all()
    # a zero anywhere is the reference's assertion, and the other elements are still inverted
    z = a.copy()
    z[n - 1] = 0
    dz = DeviceBuffer.from_numpy(z)
    rc = lib.bfs_gl_batch_inverse(dz.ptr, dc.ptr, n, 0)
    assert rc != 0 and b"batch inverse does not work when input contains a zero" in lib.bfs_last_error()
    got = dc.to_numpy()
    assert got[n - 1] == 0 and (got[:n - 1] == want[:n - 1]).all()
    # scale by an arbitrary factor, two columns with a stride
    factor = int(oracle.felt_array(SEED, n, 1)[0]) | 1
    two = DeviceBuffer.from_numpy(np.concatenate([a, a[::-1]]))
    out = DeviceBuffer(2 * n)
    _lib.check(lib.bfs_gl_scale(two.ptr, out.ptr, n, n, 2, factor, 0))
    synchronize(0)
    res = out.to_numpy()
    assert (res[:n] == oracle.scale(factor, a)).all() and (res[n:] == oracle.scale(factor, a[::-1].copy())).all()


def test_four_pass_plan_2p25(sb, oracle):
    """n = 2^25 takes four HBM passes (7 + 6 + 6 + 6 bits) and keeps the per-thread twiddle chain in its last two passes: forward,
    inverse with the n^-1 scaling, and a zero-padded coset evaluation against the oracle"""
    logn, n = 25, 1 << 25
    w = oracle.primitive_nth_root(n)
    v = oracle.felt_array(SEED + 25, 0, n)
    fwd = raw_ntt(sb, v, logn, w)
    assert (fwd == oracle.ntt(w, v)).all()
    assert (raw_ntt(sb, fwd, logn, oracle.inv(w), 1, oracle.inv(n)) == v).all()
    d = n // 4 + 3
    assert (raw_ntt(sb, v[:d], logn, w, 7, 1, n_in=d) == oracle.fast_coset_evaluate(v[:d], 7, w, n)).all()
    e = edge_values(n, 25000)                    # values next to 0, p and 2^32 through the four-pass plan as well
    assert (raw_ntt(sb, e, logn, w) == oracle.ntt(w, e)).all()
    assert (raw_ntt(sb, e[:d], logn, w, 7, 1, n_in=d) == oracle.fast_coset_evaluate(e[:d], 7, w, n)).all()


@pytest.mark.parametrize("logn", [13, 16, 17, 20, 22])
def test_multi_pass_buffer_flow(sb, oracle, logn):
    """Pass 0 of a multi-pass plan transposes from the input into the output and every later pass runs in place there (no
    intermediate buffer); when input and output overlap -- a caller transforming in place, or an output that starts inside the
    input -- passes 0 and 1 go through the library's intermediate buffer.  Same values on every route, for a batch whose
    transforms are spaced wider than n, and nothing is written between the transforms of a batch."""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer, synchronize
    lib = _lib.load()
    n = 1 << logn
    w = oracle.primitive_nth_root(n)
    batch, in_stride, out_stride = 2, n + 24, n + 8
    cols = [oracle.felt_array(SEED + 77 + b, 0, n) for b in range(batch)]
    want = [oracle.ntt(w, c) for c in cols]
    src = np.zeros(in_stride * batch, dtype=np.uint64)
    for b in range(batch):
        src[b * in_stride:b * in_stride + n] = cols[b]
    marker = np.uint64(0xDEADBEEFCAFEF00D)
    din = DeviceBuffer.from_numpy(src)
    dout = DeviceBuffer.from_numpy(np.full(out_stride * batch, marker, dtype=np.uint64))
    _lib.check(lib.bfs_gl_ntt(din.ptr, n, in_stride, dout.ptr, out_stride, logn, batch, w, 1, 1, 0)); synchronize(0)
    out = dout.to_numpy()
    for b in range(batch):
        assert (out[b * out_stride:b * out_stride + n] == want[b]).all()
        assert (out[b * out_stride + n:(b + 1) * out_stride] == marker).all()
    assert (din.to_numpy() == src).all()                                               # the input is left alone
    _lib.check(lib.bfs_gl_ntt(din.ptr, n, in_stride, din.ptr, in_stride, logn, batch, w, 1, 1, 0)); synchronize(0)      # in == out
    got = din.to_numpy()
    for b in range(batch):
        assert (got[b * in_stride:b * in_stride + n] == want[b]).all()
    # an output that starts inside the input (one transform, zero-padded coset evaluation of n / 4 coefficients)
    d = n // 4
    buf = DeviceBuffer.from_numpy(np.concatenate([cols[0][:d], np.zeros(n, dtype=np.uint64)]))
    _lib.check(lib.bfs_gl_ntt(buf.ptr, d, d, buf.ptr + 8 * (d // 2), n, logn, 1, w, 7, 1, 0)); synchronize(0)
    assert (buf.to_numpy()[d // 2:d // 2 + n] == oracle.fast_coset_evaluate(cols[0][:d], 7, w, n)).all()


def test_c_abi_argument_checks_and_stream_lifetime(sb, oracle):
    """bfs_gl_ntt refuses null pointers and batches whose transforms would overlap (BFS_ERR_BAD_ARG, nothing launched); a stream
    made by bfs_stream_create carries a multi-pass transform (its scratch buffer is keyed by the stream), and destroying it gives
    the scratch back and leaves the pools usable; the twiddle-table cache starts over after 4096 entries without disturbing
    results (4200 distinct coset shifts at 2^6, the first one re-checked at the end)."""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer, synchronize
    lib = _lib.load()
    BAD_ARG = 6
    logn, n = 8, 256
    w = lib.bfs_gl_primitive_root(logn)
    v = oracle.felt_array(SEED, 0, 2 * n)
    din, dout = DeviceBuffer.from_numpy(v), DeviceBuffer(2 * n)
    assert lib.bfs_gl_ntt(None, n, n, dout.ptr, n, logn, 1, w, 1, 1, 0) == BAD_ARG and b"null" in lib.bfs_last_error()
    assert lib.bfs_gl_ntt(din.ptr, n, n, None, n, logn, 1, w, 1, 1, 0) == BAD_ARG
    assert lib.bfs_gl_ntt(din.ptr, n, n, dout.ptr, n - 1, logn, 2, w, 1, 1, 0) == BAD_ARG and b"overlap" in lib.bfs_last_error()
    assert lib.bfs_gl_ntt(din.ptr, n, n - 1, dout.ptr, n, logn, 2, w, 1, 1, 0) == BAD_ARG
    assert lib.bfs_gl_ntt(None, 0, 0, dout.ptr, n, logn, 1, w, 1, 1, 0) == 0          # no coefficients: the zero polynomial
    synchronize(0)
    assert not dout.to_numpy(n).any()
    # a transform on a private stream (2^14: two passes, i.e. with a scratch buffer), then the stream goes away
    logm, m = 14, 1 << 14
    wm = lib.bfs_gl_primitive_root(logm)
    x = oracle.felt_array(SEED + 5, 0, m)
    want = oracle.ntt(wm, x)
    for _ in range(3):
        st = ctypes.c_void_p()
        _lib.check(lib.bfs_stream_create(ctypes.byref(st)))
        a, b = DeviceBuffer.from_numpy(x), DeviceBuffer(m)
        _lib.check(lib.bfs_gl_ntt(a.ptr, m, m, b.ptr, m, logm, 1, wm, 1, 1, st))
        _lib.check(lib.bfs_stream_synchronize(st))
        assert (b.to_numpy() == want).all()
        p = ctypes.c_void_p()
        _lib.check(lib.bfs_malloc_async(ctypes.byref(p), 1 << 16, st))
        _lib.check(lib.bfs_free_async(p, st))                   # cached with `st` as its release stream ...
        _lib.check(lib.bfs_stream_destroy(st))                  # ... which must not be waited on after this
        q = ctypes.c_void_p()
        _lib.check(lib.bfs_malloc_async(ctypes.byref(q), 1 << 16, 0))
        _lib.check(lib.bfs_free_async(q, 0))
        a.free(); b.free()
    assert lib.bfs_stream_destroy(None) == 0
    # more distinct coset shifts than the table cache holds
    k, logk = 64, 6
    wk = lib.bfs_gl_primitive_root(logk)
    y = oracle.felt_array(SEED + 6, 0, k)
    src, dst = DeviceBuffer.from_numpy(y), DeviceBuffer(k)
    first = None
    for shift in list(range(2, 4202)) + [2]:
        _lib.check(lib.bfs_gl_ntt(src.ptr, k, k, dst.ptr, k, logk, 1, wk, shift, 1, 0))
        if shift in (2, 3000, 4201):
            synchronize(0)
            got = dst.to_numpy()
            assert (got == oracle.ntt(wk, oracle.scale(shift, y))).all(), shift
            if first is None:
                first = got
    assert (got == first).all()
