"""The case table of the stream-order tests: one entry per call of include/bfstark.h that takes a `stream`, importable without a GPU.

tests/stream_order_child.py runs every case on the MI355X in two legs (order behind the caller's own held stream; nothing leaked to or
waiting for the held default stream), tests/test_stream_cases_host.py checks on the CPU that the table covers the header and that
every case's decoy input is detectable.

A case has
  name, kind        "enqueues" (the header's "only enqueues": the call returns while the stream is held, and is made twice back to
                    back with different host arguments and different device inputs) or "synchronises" (the header says so; made once);
  entries           the header functions the case calls with the stream under test;
  inputs(v)         the device operands of variant v as uint64 / uint8 arrays: v = 0, 1 the two real inputs, v = DECOY another valid
                    input of the same shape (canonical residues, 0/1 masks) that lies in the operand buffers when the call is made
                    and is replaced, in stream order, by the real input; v = WARM a third one, which the warm run and the run
                    between the legs compute from, so that the library's scratch never holds the real input's intermediates
                    when a leg starts;
  fixed()           operands the kernels use as offsets or lengths: uploaded before any hold, never a decoy;
  outputs           name -> words of device output (zeroed before every leg); a name that is also an input is read back from the
                    operand buffer (in-place calls, accumulators);
  call(lib, buf, stream, v)   makes the call(s); buf[name] is the device address of an operand, a fixed operand or an output;
                    returns the host results as {name: uint64 array} (bytes are compared through their SHA-256, four words);
  want(inp, v)      {name: expected words} from oracle/, hashlib or the host primitive the entry's parity test uses;
  select            name -> indices of the words that are compared (default: all of them; words a call leaves unwritten must stay 0
                    and are checked to do so by the child);
  sensitive         name -> indices, a subset of select, on which the decoy's reference must differ word for word (default: select).
Shapes are the smallest that take each launch shape (tests/test_gpu_buffer_contracts.py).  bfs_gl_ntt: 2^10, 2^13 and 2^17 are the one-,
two- and three-pass plans of ntt_plan.hpp; the four-pass plan starts at 2^25 = 256 MiB, where bfs_ntt_tune's routes begin, and is left out.

Calls with interior synchronisations (the FRI entries, bfs_ptree_interpolate, the scans with a host terminal): leg 1 covers the work
in front of the first synchronisation -- what follows it runs on an idle stream --, leg 2 covers all of it."""
import ctypes
import functools
import hashlib
import types
import zlib

import numpy as np

from stream_builders import PAD_MASKS, PAD_WIDTH, padded, strided

SEED = 0x57AEA
P = (1 << 64) - (1 << 32) + 1
OFFSET = 7
DECOY = 2
WARM = 3                      # a third valid input: what the library's scratch holds when a leg starts
u64, u32 = ctypes.c_uint64, ctypes.c_uint32


def oracle():
    from oracle import ref_oracle
    return ref_oracle


def ck(lib, rc):
    if rc != 0:
        raise RuntimeError("error %d: %s" % (rc, lib.bfs_last_error().decode("utf-8", "replace")))


def digest_words(data):
    return np.frombuffer(hashlib.sha256(bytes(data)).digest(), dtype=np.uint64).copy()


def as_words(data):
    """bytes or an array as whole uint64 words, zero-padded"""
    raw = np.frombuffer(bytes(data) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data).tobytes(), dtype=np.uint8)
    padded = np.zeros(-(-max(raw.size, 8) // 8) * 8, dtype=np.uint8)
    padded[:raw.size] = raw
    return padded.view(np.uint64).copy()


class Case:
    def __init__(self, name, kind, entries, inputs, call, want, outputs=None, fixed=None, select=None, sensitive=None):
        assert kind in ("enqueues", "synchronises")
        self.name, self.kind, self.entries = name, kind, tuple(entries)
        self._inputs, self.call, self._want = inputs, call, want
        self.outputs, self._fixed = dict(outputs or {}), fixed
        self.select, self.sensitive = dict(select or {}), dict(sensitive or {})
        self.base_seed = SEED + (zlib.crc32(name.encode()) & 0xFFFFF) * 8

    @property
    def variants(self):
        return (0, 1) if self.kind == "enqueues" else (0,)

    def felt(self, v, k, count):
        """`count` canonical residues, a stream of its own per (case, variant, k)"""
        return oracle().felt_array(self.base_seed + 3 * k + v + 1000003 * v, 0, count)

    def rng(self, v, k=0):
        return np.random.default_rng([self.base_seed, v, k])

    def inputs(self, v):
        return {k: np.ascontiguousarray(a) for k, a in self._inputs(self, v).items()}

    def fixed(self):
        return {k: np.ascontiguousarray(a) for k, a in (self._fixed(self) if self._fixed else {}).items()}

    def want(self, inp, v):
        return {k: np.ascontiguousarray(a, dtype=np.uint64).reshape(-1) for k, a in self._want(self, inp, v).items()}

    def selected(self, name, size):
        return np.asarray(self.select[name], dtype=np.int64) if name in self.select else np.arange(size)


CASES = []


def case(*args, **kwargs):
    c = Case(*args, **kwargs)
    assert c.name not in [x.name for x in CASES]
    CASES.append(c)
    return c


def scalars(c, v, k, count):
    return [int(x) for x in c.felt(v, 50 + k, count)]


def rows_index(batch, stride, n):
    return (np.arange(batch)[:, None] * stride + np.arange(n)[None, :]).reshape(-1)


def vadd(a, b):
    s = a + b
    s = np.where(s < a, s + np.uint64(0xFFFFFFFF), s)
    return np.where(s >= np.uint64(P), s - np.uint64(P), s)


# ------------------------------------------------------------------------------------------------ bfs_gl_ntt
def ntt_case(name, logn, n_in, batch, in_stride, out_stride, shift, scaled, in_place=False):
    n = 1 << logn

    def args(v):
        o = oracle()
        w = o.primitive_nth_root(n)
        if v == 1:
            w = o.inv(w)
        return w, (shift if shift == 1 else shift + 2 * v), ((o.inv(n) if v == 0 else 3) if scaled else 1)

    def inputs(c, v):
        return {"io" if in_place else "in": c.felt(v, 0, batch * in_stride)}

    def call(lib, buf, stream, v):
        w, s, scale = args(v)
        src = buf["io" if in_place else "in"]
        ck(lib, lib.bfs_gl_ntt(src, n_in, in_stride, buf["io" if in_place else "out"], out_stride, logn, batch, w, s, scale, stream))

    def want(c, inp, v):
        o = oracle()
        w, s, scale = args(v)
        src = inp["io" if in_place else "in"]
        out = []
        for b in range(batch):
            t = o.fast_coset_evaluate(src[b * in_stride:b * in_stride + n_in], s, w, n)
            out.append(t if scale == 1 else o.hadamard(t, np.full(n, scale, dtype=np.uint64)))
        if in_place:
            return {"io": strided(out, out_stride, src)}               # the gaps keep what the input held there
        return {"out": strided(out, out_stride, np.zeros(batch * out_stride, dtype=np.uint64))}
    assert not in_place or (in_stride == out_stride and n_in == n)
    key = "io" if in_place else "out"
    case(name, "enqueues", ["bfs_gl_ntt"], inputs, call, want, outputs={key: batch * out_stride}, select={key: rows_index(batch, out_stride, n)})


ntt_case("ntt 2^10 one pass", 10, 1 << 10, 1, 1 << 10, 1 << 10, 1, False)
ntt_case("ntt 2^13 two passes", 13, 1 << 13, 1, 1 << 13, 1 << 13, 1, False)
ntt_case("ntt 2^17 three passes", 17, 1 << 17, 1, 1 << 17, 1 << 17, 1, False)
ntt_case("ntt 2^13 of 2^9 + 1 coefficients, coset shift and post-scale", 13, (1 << 9) + 1, 1, (1 << 9) + 1, 1 << 13, 7, True)
ntt_case("ntt 2^10 batch 3 with strides", 10, 1 << 10, 3, (1 << 10) + 5, (1 << 10) + 3, 7, True)
ntt_case("ntt 2^13 in place through the library buffer", 13, 1 << 13, 1, 1 << 13, 1 << 13, 7, True, in_place=True)


# ------------------------------------------------------------------------------------------------ element-wise entry points
N_EL = 2049


def _scale():
    batch, stride = 3, N_EL + 7
    factor = lambda c, v: scalars(c, v, 0, 1)[0] | 1

    def call(lib, buf, stream, v):
        ck(lib, lib.bfs_gl_scale(buf["in"], buf["out"], N_EL, stride, batch, factor(CASE, v), stream))

    def want(c, inp, v):
        o = oracle()
        return {"out": strided([o.scale(factor(c, v), inp["in"][b * stride:b * stride + N_EL]) for b in range(batch)], stride,
                               np.zeros(batch * stride, dtype=np.uint64))}
    CASE = case("gl_scale", "enqueues", ["bfs_gl_scale"], lambda c, v: {"in": c.felt(v, 0, batch * stride)}, call, want,
                outputs={"out": batch * stride}, select={"out": rows_index(batch, stride, N_EL)})


_scale()

case("gl_mul_pointwise", "enqueues", ["bfs_gl_mul_pointwise"], lambda c, v: {"a": c.felt(v, 0, N_EL), "b": c.felt(v, 1, N_EL)},
     lambda lib, buf, stream, v: ck(lib, lib.bfs_gl_mul_pointwise(buf["a"], buf["b"], buf["out"], N_EL, stream)),
     lambda c, inp, v: {"out": oracle().hadamard(inp["a"], inp["b"])}, outputs={"out": N_EL})


def xfe_nonzero(soa):
    soa = soa.copy()
    soa[0] = np.where((soa[0] | soa[1] | soa[2]) == 0, np.uint64(1), soa[0])
    return soa


def _xfe_mul():
    sa, sb, so = N_EL + 1, N_EL + 4, N_EL + 9

    def planes(flat, stride):
        return np.stack([flat[l * stride:l * stride + N_EL] for l in range(3)])
    case("xfe_mul_pointwise", "enqueues", ["bfs_xfe_mul_pointwise"], lambda c, v: {"a": c.felt(v, 0, 3 * sa), "b": c.felt(v, 1, 3 * sb)},
         lambda lib, buf, stream, v: ck(lib, lib.bfs_xfe_mul_pointwise(buf["a"], sa, buf["b"], sb, buf["out"], so, N_EL, stream)),
         lambda c, inp, v: {"out": strided(oracle().xhadamard(planes(inp["a"], sa), planes(inp["b"], sb)), so, np.zeros(3 * so, dtype=np.uint64))},
         outputs={"out": 3 * so}, select={"out": rows_index(3, so, N_EL)})

    si = N_EL + 2

    def inv_inputs(c, v):
        return {"in": strided(xfe_nonzero(c.felt(v, 0, 3 * N_EL).reshape(3, N_EL)), si, c.felt(v, 1, 3 * si))}
    case("xfe_batch_inverse", "synchronises", ["bfs_xfe_batch_inverse"], inv_inputs,
         lambda lib, buf, stream, v: ck(lib, lib.bfs_xfe_batch_inverse(buf["in"], si, buf["out"], so, N_EL, stream)),
         lambda c, inp, v: {"out": strided(oracle().xbatch_inverse(planes(inp["in"], si)), so, np.zeros(3 * so, dtype=np.uint64))},
         outputs={"out": 3 * so}, select={"out": rows_index(3, so, N_EL)})


_xfe_mul()

case("gl_batch_inverse", "synchronises", ["bfs_gl_batch_inverse"], lambda c, v: {"in": np.where(c.felt(v, 0, N_EL) == 0, np.uint64(1), c.felt(v, 0, N_EL))},
     lambda lib, buf, stream, v: ck(lib, lib.bfs_gl_batch_inverse(buf["in"], buf["out"], N_EL, stream)),
     lambda c, inp, v: {"out": oracle().batch_inverse(inp["in"])}, outputs={"out": N_EL})


# ------------------------------------------------------------------------------------------------ subproduct tree
def zerofier_of(points):
    """coefficients of prod (X - x_i), lowest first, by a product tree over oracle.fast_multiply"""
    o = oracle()
    polys = [[o.neg(int(x)), 1] for x in points]
    order = 1 << 14
    root = o.primitive_nth_root(order)
    while len(polys) > 1:
        polys = [o.fast_multiply(polys[k], polys[k + 1], root, order) if k + 1 < len(polys) else polys[k] for k in range(0, len(polys), 2)]
    return np.array(polys[0], dtype=np.uint64)


def evaluate_at(coeffs, points):
    """Horner over all points at once, in the oracle's arithmetic"""
    o = oracle()
    acc = np.zeros(len(points), dtype=np.uint64)
    for cf in coeffs[::-1]:
        acc = vadd(o.hadamard(acc, points), np.full(len(points), cf, dtype=np.uint64))
    return acc


def interpolate_through(points, values):
    """Lagrange on Python integers: the polynomial of degree < n with P(x_i) = v_i"""
    n = len(points)
    xs, z = [int(x) for x in points], [int(c) for c in zerofier_of(points)]
    out = [0] * n
    for i in range(n):
        q, carry = [0] * n, 0                     # z / (X - x_i) by synthetic division
        for k in range(n, 0, -1):
            carry = (z[k] + carry * xs[i]) % P
            q[k - 1] = carry
        den = 1
        for j in range(n):
            if j != i:
                den = den * (xs[i] - xs[j]) % P
        w = int(values[i]) * pow(den, P - 2, P) % P
        for k in range(n):
            out[k] = (out[k] + w * q[k]) % P
    return np.array(out, dtype=np.uint64)


def ptree_case(n):
    batch, m, out_stride = 2, n + 1, n + 5
    in_stride = m + 2

    def inputs(c, v):
        pts = c.felt(v, 0, n)
        assert len(set(pts.tolist())) == n
        return {"points": pts, "coeffs": c.felt(v, 1, batch * in_stride)}

    def call(lib, buf, stream, v):
        tree = ctypes.c_void_p()
        ck(lib, lib.bfs_ptree_build(buf["points"], n, stream, ctypes.byref(tree)))
        ck(lib, lib.bfs_ptree_zerofier(tree, buf["zerofier"], stream))
        ck(lib, lib.bfs_ptree_evaluate(tree, buf["coeffs"], m, in_stride, batch, buf["values"], out_stride, stream))
        ck(lib, lib.bfs_ptree_free(tree, stream))

    def want(c, inp, v):
        vals = [evaluate_at(inp["coeffs"][b * in_stride:b * in_stride + m], inp["points"]) for b in range(batch)]
        return {"zerofier": zerofier_of(inp["points"]), "values": strided(vals, out_stride, np.zeros(batch * out_stride, dtype=np.uint64))}
    case("ptree build, zerofier, evaluate, free n=%d" % n, "enqueues", ["bfs_ptree_build", "bfs_ptree_zerofier", "bfs_ptree_evaluate", "bfs_ptree_free"],
         inputs, call, want, outputs={"zerofier": n + 1, "values": batch * out_stride},
         select={"values": rows_index(batch, out_stride, n)}, sensitive={"zerofier": np.arange(n)})          # the leading coefficient is 1


ptree_case(65)
ptree_case(4097)


def _interpolate():
    n, batch = 65, 2
    in_stride, out_stride = n + 2, n + 5

    def call(lib, buf, stream, v):
        tree = ctypes.c_void_p()
        ck(lib, lib.bfs_ptree_build(buf["points"], n, stream, ctypes.byref(tree)))
        ck(lib, lib.bfs_ptree_interpolate(tree, buf["values"], in_stride, batch, buf["out"], out_stride, stream))
        ck(lib, lib.bfs_ptree_free(tree, stream))

    def want(c, inp, v):
        polys = [interpolate_through(inp["points"], inp["values"][b * in_stride:b * in_stride + n]) for b in range(batch)]
        return {"out": strided(polys, out_stride, np.zeros(batch * out_stride, dtype=np.uint64))}
    case("ptree_interpolate n=65", "synchronises", ["bfs_ptree_interpolate"],
         lambda c, v: {"points": c.felt(v, 0, n), "values": c.felt(v, 1, batch * in_stride)}, call, want,
         outputs={"out": batch * out_stride}, select={"out": rows_index(batch, out_stride, n)})


_interpolate()


# ------------------------------------------------------------------------------------------------ FRI folds
def fold_case(entry, k):
    import fri_folding_model as folding_model
    log_n = 10
    n = 1 << log_n
    q = n >> k
    so = q + 9

    def call(lib, buf, stream, v):
        alpha = (u64 * 3)(*scalars(CASE, v, 0, 3))
        omega = oracle().primitive_nth_root(n)
        if entry == "bfs_xfe_fold":
            ck(lib, lib.bfs_xfe_fold(buf["in"], n, buf["out"], so, log_n, alpha, OFFSET, omega, stream))
        else:
            ck(lib, lib.bfs_xfe_fold_multi(buf["in"], n, buf["out"], so, log_n, k, alpha, OFFSET, omega, stream))

    def want(c, inp, v):
        o = oracle()
        got, _, _ = folding_model.fold_round(o, inp["in"].reshape(3, n), scalars(c, v, 0, 3), OFFSET, o.primitive_nth_root(n), k)
        return {"out": strided(got, so, np.zeros(3 * so, dtype=np.uint64))}
    CASE = case("%s by %d" % (entry[4:], 1 << k), "enqueues", [entry], lambda c, v: {"in": c.felt(v, 0, 3 * n)}, call, want,
                outputs={"out": 3 * so}, select={"out": rows_index(3, so, q)})


fold_case("bfs_xfe_fold", 1)
fold_case("bfs_xfe_fold_multi", 2)
fold_case("bfs_xfe_fold_multi", 3)


# ------------------------------------------------------------------------------------------------ Merkle trees
def node_words(leaves):
    """indices of the words of digests 1 .. npo2 + leaves - 1 (digest 0 and the slots of absent leaves are not written)"""
    npo2 = 1 << max(leaves - 1, 0).bit_length()
    return npo2, np.arange(8, 8 * (npo2 + leaves))


def live_node_words(leaves):
    """the words of the digests that depend on a leaf: node k of level l spans the leaves from (k << (depth - l)) - npo2 on; a node
    over absent leaves only is a constant (the hash of 32 zero bytes, and its ancestors')"""
    npo2 = 1 << max(leaves - 1, 0).bit_length()
    depth = npo2.bit_length() - 1
    live = [k for k in range(1, npo2 + leaves) if (k << (depth - (k.bit_length() - 1))) - npo2 < leaves]
    return (np.array(live)[:, None] * 8 + np.arange(8)[None, :]).reshape(-1)


def nodes_as_words(nodes, npo2, leaves):
    raw = b"".join(bytes(nodes[k]) if 1 <= k < npo2 + leaves else bytes(64) for k in range(2 * npo2))
    return np.frombuffer(raw, dtype=np.uint64)


N_MERKLE = 257


def _merkle():
    import commitment_check as cc
    n, stride = N_MERKLE, N_MERKLE + 3
    npo2, idx = node_words(n)

    def soa(inp):
        return np.stack([inp["codeword"][l * stride:l * stride + n] for l in range(3)])
    case("merkle_build_xfe", "enqueues", ["bfs_merkle_build_xfe"], lambda c, v: {"codeword": c.felt(v, 0, 3 * stride)},
         lambda lib, buf, stream, v: ck(lib, lib.bfs_merkle_build_xfe(buf["codeword"], stride, n, buf["nodes"], stream)),
         lambda c, inp, v: {"nodes": nodes_as_words(oracle().xfe_merkle(soa(inp))[0].nodes, npo2, n)},
         outputs={"nodes": 16 * npo2}, select={"nodes": idx}, sensitive={"nodes": live_node_words(n)})
    case("merkle_build_bfe", "enqueues", ["bfs_merkle_build_bfe"], lambda c, v: {"values": c.felt(v, 0, n)},
         lambda lib, buf, stream, v: ck(lib, lib.bfs_merkle_build_bfe(buf["values"], n, buf["nodes"], stream)),
         lambda c, inp, v: {"nodes": nodes_as_words(oracle().MerkleOracle([cc.bfe_preimage(inp["values"], i) for i in range(n)]).nodes, npo2, n)},
         outputs={"nodes": 16 * npo2}, select={"nodes": idx}, sensitive={"nodes": live_node_words(n)})

    def layout(c):
        rng = c.rng(9)
        lengths = rng.integers(1, 300, n).astype(np.uint32)
        words = (lengths.astype(np.uint64) + np.uint64(7)) // np.uint64(8)
        offsets = np.zeros(n, dtype=np.uint64)
        np.cumsum(words[:-1], out=offsets[1:])
        return lengths, offsets, int(words.sum())

    def bytes_want(c, inp, v):
        lengths, offsets, _ = layout(c)
        raw = inp["data"].view(np.uint8)
        leaves = [raw[int(off) * 8:int(off) * 8 + int(k)].tobytes() for k, off in zip(lengths, offsets)]
        return {"nodes": nodes_as_words(oracle().MerkleOracle(leaves).nodes, npo2, n)}
    case("merkle_build_bytes", "enqueues", ["bfs_merkle_build_bytes"],
         lambda c, v: {"data": c.rng(v).integers(0, 1 << 63, layout(c)[2], dtype=np.uint64)},
         lambda lib, buf, stream, v: ck(lib, lib.bfs_merkle_build_bytes(buf["data"], buf["offsets"], buf["lengths"], n, buf["nodes"], stream)),
         bytes_want, outputs={"nodes": 16 * npo2}, select={"nodes": idx}, sensitive={"nodes": live_node_words(n)},
         fixed=lambda c: {"offsets": layout(c)[1], "lengths": as_words(layout(c)[0].tobytes())})

    depth = 8

    def open_call(lib, buf, stream, v):
        path = np.zeros(8 * depth, dtype=np.uint64)
        ck(lib, lib.bfs_merkle_open(buf["nodes"], depth, 77 + v, path.ctypes.data, stream))
        return {"path": path}
    case("merkle_open", "synchronises", ["bfs_merkle_open"], lambda c, v: {"nodes": c.rng(v).integers(0, 1 << 63, 16 << depth, dtype=np.uint64)},
         open_call, lambda c, inp, v: {"path": np.concatenate([inp["nodes"][8 * (k ^ 1):8 * (k ^ 1) + 8] for k in
                                                                [((1 << depth) | 77 + v) >> lvl for lvl in range(depth)]])})

    import fri_coset_model as coset_model
    N, a = 1 << 10, 4
    cstride = N + 8
    case("merkle_build_xfe_cosets", "synchronises", ["bfs_merkle_build_xfe_cosets"], lambda c, v: {"codeword": c.felt(v, 0, 3 * cstride)},
         lambda lib, buf, stream, v: ck(lib, lib.bfs_merkle_build_xfe_cosets(buf["codeword"], cstride, N, 2, buf["nodes"], stream)),
         lambda c, inp, v: {"nodes": nodes_as_words(coset_model.tree_nodes(oracle(), inp["codeword"].reshape(3, cstride), N, a), N // a, N // a)},
         outputs={"nodes": 16 * (N // a)}, select={"nodes": node_words(N // a)[1]})


_merkle()


def rows_case(entry, salts_on_device):
    """two extension and two base columns of 2^10 rows, the 2^8 rows from 384 on (the whole columns for bfs_merkle_build_rows)"""
    import commitment_check as cc
    from stark_brainfuck_amd import _lib
    whole = entry == "bfs_merkle_build_rows"
    total = 1 << 8 if whole else 1 << 10
    n, first = 1 << 8, 0 if whole else 384
    npo2, idx = node_words(n)
    shapes = [3, 1, 3, 1]

    def inputs(c, v):
        inp = {"column%d" % k: c.felt(v, k, w * total) for k, w in enumerate(shapes)}
        if salts_on_device:
            inp["salts"] = c.rng(v, 7).integers(0, 1 << 63, 3 * n, dtype=np.uint64)
        return inp

    def host_salts(c, v):
        return c.rng(v, 7).integers(0, 1 << 63, 3 * n, dtype=np.uint64).tobytes()

    def call(lib, buf, stream, v):
        rc = (_lib.RowColumn * 4)()
        for k, w in enumerate(shapes):
            rc[k].d_values, rc[k].is_ext, rc[k].field_id = buf["column%d" % k] + 8 * first, int(w == 3), 0
        keep = None if salts_on_device else ctypes.create_string_buffer(host_salts(CASE, v), 24 * n)
        salts = buf["salts"] if salts_on_device else ctypes.cast(keep, ctypes.c_void_p)
        if entry == "bfs_merkle_build_rows":
            ck(lib, lib.bfs_merkle_build_rows(rc, 4, n, salts, int(salts_on_device), buf["nodes"], stream))
        elif entry == "bfs_merkle_build_rows_range":
            ck(lib, lib.bfs_merkle_build_rows_range(rc, 4, n, total, salts, int(salts_on_device), buf["nodes"], stream))
        else:
            root = ctypes.create_string_buffer(64)
            ck(lib, lib.bfs_merkle_build_rows_root(rc, 4, n, total, salts, int(salts_on_device), buf["nodes"], root, stream))
            return {"root": as_words(root.raw)}

    def want(c, inp, v):
        salts = inp["salts"].tobytes() if salts_on_device else host_salts(c, v)
        window = [np.ascontiguousarray((inp["column%d" % k].reshape(3, total) if w == 3 else inp["column%d" % k])[..., first:first + n])
                  for k, w in enumerate(shapes)]
        tree = oracle().MerkleOracle([cc.row_preimage(window, i, salts[24 * i:24 * i + 24]) for i in range(n)])
        out = {"nodes": nodes_as_words(tree.nodes, npo2, n)}
        if entry == "bfs_merkle_build_rows_root":
            out["root"] = as_words(tree.nodes[1])
        return out
    CASE = case("%s, salts %s" % (entry[4:], "in HBM" if salts_on_device else "on the host"), "synchronises", [entry], inputs, call, want,
                outputs={"nodes": 16 * npo2}, select={"nodes": idx})


rows_case("bfs_merkle_build_rows_root", True)
rows_case("bfs_merkle_build_rows_root", False)
rows_case("bfs_merkle_build_rows_range", False)
rows_case("bfs_merkle_build_rows", True)


# ------------------------------------------------------------------------------------------------ random fills
def _fills():
    seed = lambda v: bytes(range(50 + 40 * v, 82 + 40 * v))
    nwords, count = 8008, 1000
    case("random_fill", "enqueues", ["bfs_random_fill"], lambda c, v: {},
         lambda lib, buf, stream, v: ck(lib, lib.bfs_random_fill(seed(v), buf["out"], nwords, stream)),
         lambda c, inp, v: {"out": np.frombuffer(b"".join(hashlib.blake2b(seed(v) + j.to_bytes(8, "little")).digest() for j in range(nwords // 8)), dtype=np.uint64)},
         outputs={"out": nwords})

    def sample_want(c, inp, v):
        blocks = (27 * count + 62) // 63
        stream = b"".join(hashlib.blake2b(seed(v) + b.to_bytes(8, "little")).digest()[:63] for b in range(blocks))
        planes = [[int.from_bytes(stream[27 * i + 9 * j:27 * i + 9 * j + 9], "big") % P for i in range(count)] for j in range(3)]
        return {"out": strided(np.array(planes, dtype=np.uint64), count + 3, np.zeros(3 * (count + 3), dtype=np.uint64))}
    case("xfe_sample_fill", "enqueues", ["bfs_xfe_sample_fill"], lambda c, v: {},
         lambda lib, buf, stream, v: ck(lib, lib.bfs_xfe_sample_fill(seed(v), buf["out"], count, count + 3, stream)), sample_want,
         outputs={"out": 3 * (count + 3)}, select={"out": rows_index(3, count + 3, count)})


_fills()


# ------------------------------------------------------------------------------------------------ trace padding
PAD_HEIGHTS, PAD_ROWS = [512, 64, 256, 8, 2], [300, 64, 100, 5, 1]


def _trace_pad():
    from stark_brainfuck_amd import _lib

    def inputs(c, v):
        inp = {}
        for t, k in enumerate(PAD_ROWS):
            stride = PAD_WIDTH[t] + 2
            rng = c.rng(v, t)
            rows = rng.integers(0, 1 << 63, (k, stride), dtype=np.uint64)
            if t == 0:            # current instructions: zero, ',', '.' and others, so that the three masks are not constant
                rows[:, 2] = rng.choice(np.array([0, ord(","), ord("."), ord("+")], dtype=np.uint64), k)
            if t == 1:
                rows[:, 0] = np.sort(rng.integers(0, k // 3, k).astype(np.uint64))
                rows[:, 1] = rng.choice(np.array([0, ord("+")], dtype=np.uint64), k)
            inp["rows%d" % t] = rows.reshape(-1)
        return inp

    outputs = {}
    for t, h in enumerate(PAD_HEIGHTS):
        outputs["out%d" % t] = PAD_WIDTH[t] * h
        for m in range(PAD_MASKS[t]):
            outputs["mask%d_%d" % (t, m)] = -(-h // 8)

    def call(lib, buf, stream, v):
        structs = (_lib.TracePadTable * 5)()
        for t, (h, k) in enumerate(zip(PAD_HEIGHTS, PAD_ROWS)):
            s = structs[t]
            s.d_rows, s.rows, s.row_stride, s.height = buf["rows%d" % t], k, PAD_WIDTH[t] + 2, h
            s.d_out, s.kind, s.width = buf["out%d" % t], t, PAD_WIDTH[t]
            s.d_mask0, s.d_mask1, s.d_mask2 = [buf.get("mask%d_%d" % (t, m)) for m in range(3)]
        ck(lib, lib.bfs_trace_pad(structs, 5, stream))

    def want(c, inp, v):
        out = {}
        for t, (h, k) in enumerate(zip(PAD_HEIGHTS, PAD_ROWS)):
            cols, masks = padded(t, inp["rows%d" % t].reshape(k, PAD_WIDTH[t] + 2), PAD_WIDTH[t], h)
            out["out%d" % t] = np.array(cols, dtype=np.uint64).reshape(-1)
            for m in range(PAD_MASKS[t]):
                out["mask%d_%d" % (t, m)] = as_words(bytes(masks[m]))
        return out
    # a decoy is told apart by the words of the real rows; padding rows repeat constants, and a mask word is eight 0/1 bytes
    sensitive = {"out%d" % t: rows_index(PAD_WIDTH[t], h, k) for t, (h, k) in enumerate(zip(PAD_HEIGHTS, PAD_ROWS))}
    sensitive["out0"] = np.array([i for i in sensitive["out0"] if i // PAD_HEIGHTS[0] != 2])        # the instruction column has four values
    sensitive["out1"] = np.array([i for i in sensitive["out1"] if i // PAD_HEIGHTS[1] == 2])        # sorted addresses and two instructions repeat
    for t in range(3):
        for m in range(PAD_MASKS[t]):
            sensitive["mask%d_%d" % (t, m)] = np.array([], dtype=np.int64)
    case("trace_pad, five tables", "enqueues", ["bfs_trace_pad"], inputs, call, want, outputs=outputs, sensitive=sensitive)


_trace_pad()


# ------------------------------------------------------------------------------------------------ pointwise prover kernels
LOG_N = 9
N = 1 << LOG_N
HEIGHT = 64


@functools.lru_cache(maxsize=None)
def pointwise():
    """the reference of tests/test_gpu_pointwise_edges.py: stark_brainfuck_amd/air.py on Python integers"""
    import test_gpu_pointwise_edges as pe
    assert (pe.LOG_N, pe.N, pe.OFFSET, pe.HEIGHT) == (LOG_N, N, OFFSET, HEIGHT)
    return pe


def obj(a):
    return np.array([int(x) for x in a], dtype=object)


def triple_planes(flat, n=N):
    return tuple(obj(flat[l * n:(l + 1) * n]) for l in range(3))


def words_of(planes):
    return np.array([int(x) % P for l in planes for x in (l if isinstance(l, np.ndarray) else [l] * N)], dtype=np.uint64)


def flat3(triples):
    return (u64 * (3 * len(triples)))(*[int(x) for t in triples for x in t])


AIR_TABLE = 2                      # the memory table: four base columns, one extension column


@functools.lru_cache(maxsize=None)
def air_shape():
    return pointwise().Shape(AIR_TABLE, HEIGHT)


def air_ops(c, inp, v):
    shape = air_shape()
    s = scalars(c, v, 1, 3 * (11 + 5 + 1 + 1 + 2 * shape.nterm))
    tr = [tuple(s[3 * k:3 * k + 3]) for k in range(len(s) // 3)]
    ops = types.SimpleNamespace(shape=shape, name="stream", challenges=tr[:11], terminals=tr[11:16], params=tr[16], w0=tr[17],
                                weights=[(tr[18 + 2 * k], tr[19 + 2 * k]) for k in range(shape.nterm)])
    if inp is not None:
        ops.base = [obj(inp["base"][k * N:(k + 1) * N]) for k in range(shape.bw)]
        ops.ext = [triple_planes(inp["ext"][3 * k * N:3 * (k + 1) * N]) for k in range(shape.xw)]
        if "randomizer" in inp:
            ops.randomizer = triple_planes(inp["randomizer"])
        if "acc" in inp:
            ops.seeded = triple_planes(inp["acc"])
    return shape, ops


def air_args(shape, ops):
    return (LOG_N, shape.unit_distance, shape.height, shape.omicron_inv, OFFSET, pointwise().OMEGA, flat3(ops.challenges), flat3(ops.terminals),
            flat3([ops.params]))


def weight_array(shape, ops, shifts):
    from stark_brainfuck_amd import _lib
    ws = (_lib.CombWeight * shape.nterm)()
    for w, (wa, wb), s in zip(ws, ops.weights, shifts):
        w.wa, w.wb, w.shift = (u64 * 3)(*wa), (u64 * 3)(*wb), s
    return ws


def _air():
    pe = pointwise
    widths = air_shape

    def base_ext(c, v):
        s = widths()
        return {"base": c.felt(v, 0, s.bw * N), "ext": c.felt(v, 1, 3 * s.xw * N)}

    def q_call(lib, buf, stream, v):
        shape, ops = air_ops(Q, None, v)
        ck(lib, lib.bfs_air_quotients(AIR_TABLE, buf["base"], buf["ext"], buf["out"], *air_args(shape, ops), stream))

    def q_want(c, inp, v):
        shape, ops = air_ops(c, inp, v)
        return {"out": words_of([l for q in pe().quotients(shape, ops, ops.params) for l in q])}
    # a constraint over base columns only has a base-field value: limbs 1 and 2 of its quotient are zero whatever the input
    base_only = sum(len(cs) for _, cs in widths().air.base())
    planes = [3 * q for q in range(base_only)] + list(range(3 * base_only, 3 * widths().nq))
    Q = case("air_quotients, memory table", "enqueues", ["bfs_air_quotients"], base_ext, q_call, q_want, outputs={"out": 3 * widths().nq * N},
             sensitive={"out": (rows_index(len(planes), N, N).reshape(len(planes), N) % N + np.array(planes)[:, None] * N).reshape(-1)})

    def combine_want(c, inp, v, start):
        shape, ops = air_ops(c, inp, v)
        terms = [(col, 0, 0) for col in ops.base] + list(ops.ext) + pe().quotients(shape, ops, ops.params)
        begin = pe().xmul(ops.w0, ops.randomizer) if start == "randomizer" else ops.seeded
        return pe().combination(shape, ops, terms, pe().shifts_for(shape, "generic" if v == 0 else "ungrouped"), begin)

    def c_call(lib, buf, stream, v):
        shape, ops = air_ops(C, None, v)
        ws = weight_array(shape, ops, pe().shifts_for(shape, "generic" if v == 0 else "ungrouped"))
        ck(lib, lib.bfs_air_combine(AIR_TABLE, buf["base"], buf["ext"], *air_args(shape, ops), ws, buf["randomizer"], flat3([ops.w0]), buf["acc"],
                                    None, stream))
    C = case("air_combine from the randomizer, memory table", "enqueues", ["bfs_air_combine"],
             lambda c, v: dict(base_ext(c, v), randomizer=c.felt(v, 2, 3 * N)), c_call,
             lambda c, inp, v: {"acc": words_of(combine_want(c, inp, v, "randomizer"))}, outputs={"acc": 3 * N})

    first, count = 250, 12
    inside = (np.arange(3 * N) % N >= first) & (np.arange(3 * N) % N < first + count)

    def r_call(lib, buf, stream, v):
        shape, ops = air_ops(R, None, v)
        ws = weight_array(shape, ops, pe().shifts_for(shape, "generic" if v == 0 else "ungrouped"))
        ck(lib, lib.bfs_air_combine_rows(AIR_TABLE, buf["base"], buf["ext"], *air_args(shape, ops), ws, None, None, buf["acc"], None, first, count, stream))
    R = case("air_combine_rows onto an accumulator, memory table", "enqueues", ["bfs_air_combine_rows"],
             lambda c, v: dict(base_ext(c, v), acc=c.felt(v, 3, 3 * N)), r_call,
             lambda c, inp, v: {"acc": np.where(inside, words_of(combine_want(c, inp, v, "seeded")), inp["acc"])}, outputs={"acc": 3 * N})


_air()


def points():
    return pointwise().POINTS


def _difference():
    pe = pointwise

    def quotient(inp):
        lhs, rhs = triple_planes(inp["lhs"]), triple_planes(inp["rhs"])
        return pe().xscale(tuple((a - b) % P for a, b in zip(lhs, rhs)), pe().inverses(points() - 1))
    lr = lambda c, v: {"lhs": c.felt(v, 0, 3 * N), "rhs": c.felt(v, 1, 3 * N)}
    case("difference_quotient", "enqueues", ["bfs_difference_quotient"], lr,
         lambda lib, buf, stream, v: ck(lib, lib.bfs_difference_quotient(buf["lhs"], buf["rhs"], buf["out"], LOG_N, OFFSET, pe().OMEGA, stream)),
         lambda c, inp, v: {"out": words_of(quotient(inp))}, outputs={"out": 3 * N})

    def weight(c, v):
        s = scalars(c, v, 1, 6)
        return tuple(s[:3]), tuple(s[3:]), (5, N + 3)[v]

    def combined(c, inp, v):
        wa, wb, shift = weight(c, v)
        power = np.array([pow(int(x), shift, P) for x in points()], dtype=object)
        return words_of(pe().xadd(triple_planes(inp["acc"]), pe().xmul(pe().xadd(wa, pe().xscale(wb, power)), quotient(inp))))

    def struct(c, v):
        from stark_brainfuck_amd import _lib
        wa, wb, shift = weight(c, v)
        return _lib.CombWeight((u64 * 3)(*wa), (u64 * 3)(*wb), shift)
    lra = lambda c, v: dict(lr(c, v), acc=c.felt(v, 2, 3 * N))
    D = case("difference_combine", "enqueues", ["bfs_difference_combine"], lra,
             lambda lib, buf, stream, v: ck(lib, lib.bfs_difference_combine(buf["lhs"], buf["rhs"], LOG_N, OFFSET, pe().OMEGA, ctypes.byref(struct(D, v)),
                                                                          buf["acc"], None, stream)),
             lambda c, inp, v: {"acc": combined(c, inp, v)}, outputs={"acc": 3 * N})
    first, count = 250, 12
    inside = (np.arange(3 * N) % N >= first) & (np.arange(3 * N) % N < first + count)
    DR = case("difference_combine_rows", "enqueues", ["bfs_difference_combine_rows"], lra,
              lambda lib, buf, stream, v: ck(lib, lib.bfs_difference_combine_rows(buf["lhs"], buf["rhs"], LOG_N, OFFSET, pe().OMEGA,
                                                                                ctypes.byref(struct(DR, v)), buf["acc"], None, first, count, stream)),
              lambda c, inp, v: {"acc": np.where(inside, combined(c, inp, v), inp["acc"])}, outputs={"acc": 3 * N})

    # zerofier inverses: no device operand; the two calls of a pair invert different denominators
    def specs(c, v):
        return [(0, 1), (0, scalars(c, v, 0, 1)[0]), (1, 6 - v)]

    def z_want(c, inp, v):
        x = points()
        dens = [(np.array([pow(int(e), 1 << val, P) for e in x], dtype=object) - 1) % P if is_power else (x - val) % P for is_power, val in specs(c, v)]
        return np.concatenate([words_of([pe().inverses(d)]) for d in dens])

    def z_args(c, v):
        sp = specs(c, v)
        return (LOG_N, OFFSET, pe().OMEGA, 3, (u32 * 3)(*[s[0] for s in sp]), (u64 * 3)(*[s[1] for s in sp]))
    Z = case("zerofier_inverses", "enqueues", ["bfs_zerofier_inverses"], lambda c, v: {},
             lambda lib, buf, stream, v: ck(lib, lib.bfs_zerofier_inverses(*z_args(Z, v), buf["out"], stream)),
             lambda c, inp, v: {"out": z_want(c, inp, v)}, outputs={"out": 3 * N})
    ZR = case("zerofier_inverses_rows", "enqueues", ["bfs_zerofier_inverses_rows"], lambda c, v: {},
              lambda lib, buf, stream, v: ck(lib, lib.bfs_zerofier_inverses_rows(*z_args(ZR, v), buf["out"], first, count, stream)),
              lambda c, inp, v: {"out": np.where(inside, z_want(c, inp, v), np.uint64(0))}, outputs={"out": 3 * N},
              select={"out": np.flatnonzero(inside)})


_difference()


def _randomize_and_support():
    h, batch = 64, 3
    stride = h + 3

    def want(c, inp, v):
        o = oracle()
        point = o.primitive_nth_root(N)
        values = scalars(c, v, 1, batch)
        out = inp["coeffs"].copy()
        den = o.inv(o.sub(o.power(point, h), 1))
        for b in range(batch):
            f = out[b * stride:(b + 1) * stride]
            at = 0
            for cf in f[:h][::-1]:
                at = o.add(o.mul(at, point), int(cf))
            cc_ = o.mul(o.sub(values[b], at), den)
            f[0], f[h] = o.sub(int(f[0]), cc_), cc_
        return {"coeffs": out}
    R = case("poly_randomize", "enqueues", ["bfs_poly_randomize"], lambda c, v: {"coeffs": c.felt(v, 0, batch * stride)},
             lambda lib, buf, stream, v: ck(lib, lib.bfs_poly_randomize(buf["coeffs"], stride, h, batch, oracle().primitive_nth_root(N),
                                                                      (u64 * batch)(*scalars(R, v, 1, batch)), stream)),
             want, outputs={"coeffs": batch * stride}, select={"coeffs": rows_index(batch, stride, h + 1)})

    length = 4099

    def sparse(c, v):
        """polynomial b of variant v has non-zero coefficients at the multiples of 2^(1 + v + b) only, and a constant one iff b is even:
        every mask word depends on the variant"""
        flat = np.zeros(batch * (length + 3), dtype=np.uint64)
        for b in range(batch):
            step = 1 << (1 + v + b)
            f = flat[b * (length + 3):b * (length + 3) + length]
            f[step::step] = c.felt(v, b, len(f[step::step])) | np.uint64(1)
            f[0] = (b + v) % 2
        return {"coeffs": flat}

    def s_call(lib, buf, stream, v):
        masks = (u64 * batch)()
        ck(lib, lib.bfs_poly_support(buf["coeffs"], length + 3, length, batch, masks, stream))
        return {"masks": np.array(list(masks), dtype=np.uint64)}

    def s_want(c, inp, v):
        out = []
        for b in range(batch):
            f = inp["coeffs"][b * (length + 3):b * (length + 3) + length]
            m = (1 << 63) if f[0] else 0
            for j in np.flatnonzero(f[1:]) + 1:
                m |= int(j) & -int(j)
            out.append(m)
        return {"masks": np.array(out, dtype=np.uint64)}
    case("poly_support", "synchronises", ["bfs_poly_support"], sparse, s_call, s_want)


_randomize_and_support()


def _combination():
    pe = pointwise

    def parts(c, v):
        s = scalars(c, v, 5, 3 + 3 * 6)
        tr = [tuple(s[3 * k:3 * k + 3]) for k in range(7)]
        return tr[0], [(tr[1 + 2 * k], tr[2 + 2 * k], (3, N + 5, 40)[k]) for k in range(3)]

    def call(lib, buf, stream, v):
        from stark_brainfuck_amd import _lib
        w0, ws = parts(CASE, v)
        sources = (_lib.CombSource * 3)()
        for src, name, is_ext, (wa, wb, s) in zip(sources, ("base", "ext0", "ext1"), (0, 1, 1), ws):
            src.ptr, src.is_ext, src.pad, src.shift, src.wa, src.wb = buf[name], is_ext, 0, s, (u64 * 3)(*wa), (u64 * 3)(*wb)
        ck(lib, lib.bfs_combination(sources, 3, buf["randomizer"], flat3([w0]), buf["out"], LOG_N, OFFSET, pe().OMEGA, stream))

    def want(c, inp, v):
        w0, ws = parts(c, v)
        acc = pe().xmul(w0, triple_planes(inp["randomizer"]))
        values = [(obj(inp["base"]), 0, 0), triple_planes(inp["ext0"]), triple_planes(inp["ext1"])]
        for (wa, wb, s), val in zip(ws, values):
            power = np.array([pow(int(x), s, P) for x in points()], dtype=object)
            acc = pe().xadd(acc, pe().xmul(pe().xadd(wa, pe().xscale(wb, power)), val))
        return {"out": words_of([pe().full(l) for l in acc])}
    CASE = case("combination", "synchronises", ["bfs_combination"],
                lambda c, v: {"base": c.felt(v, 0, N), "ext0": c.felt(v, 1, 3 * N), "ext1": c.felt(v, 2, 3 * N), "randomizer": c.felt(v, 3, 3 * N)},
                call, want, outputs={"out": 3 * N})


_combination()


def _gather():
    words = 4096
    plan = [(5, 3, 7), (1000, 1, 1), (17, 8, 500), (4095, 1, 1)]                  # (first word, nwords, stride)

    def call(lib, buf, stream, v):
        from stark_brainfuck_amd import _lib
        reqs = (_lib.GatherRequest * len(plan))()
        for r, (first, nwords, stride) in zip(reqs, plan):
            r.d_base, r.nwords, r.stride, r.out_offset = buf["data"] + 8 * (first + v), nwords, stride, 0
        out = np.zeros(sum(p[1] for p in plan), dtype=np.uint64)
        ck(lib, lib.bfs_gather(reqs, len(plan), out.ctypes.data, stream))
        return {"out": out}
    case("gather", "synchronises", ["bfs_gather"], lambda c, v: {"data": c.felt(v, 0, words + 8)}, call,
         lambda c, inp, v: {"out": np.concatenate([inp["data"][first + v:first + v + nwords * stride:stride][:nwords] for first, nwords, stride in plan])})


_gather()


def _air_check():
    rows, ld = 64, 70

    def call(lib, buf, stream, v):
        from stark_brainfuck_amd import _lib, air
        nq = sum(len(cs) for _, cs in air.TABLE_AIRS[AIR_TABLE].base())
        out = (_lib.AirViolation * nq)()
        ck(lib, lib.bfs_air_check(AIR_TABLE, 0, buf["base"], None, rows, ld, None, None, None, out, stream))
        return {"violations": np.array([x for o in out for x in (o.first_row, o.count)], dtype=np.uint64)}

    def want(c, inp, v):
        from stark_brainfuck_amd import air
        import test_gpu_air_check as ac
        width = air.TABLE_AIRS[AIR_TABLE].base_width
        base = np.array([[int(x) for x in inp["base"][k * ld:k * ld + rows]] for k in range(width)], dtype=object)
        return {"violations": np.array([x for pair in ac.HostAir(air.TABLE_AIRS[AIR_TABLE], base, None, 0).expected() for x in pair], dtype=np.uint64)}

    def inputs(c, v):
        """residues behind a run of zero rows whose length is the variant's: rows of zeros keep the transition constraints, so where the
        first failure lies and how many rows fail tells the variants apart in the words of five transition constraints; the three
        boundary constraints hold for every variant and the sixth transition constraint fails on all 63 pairs of residues or zeros"""
        base = c.felt(v, 0, 4 * ld).reshape(4, ld)
        base[:, :5 + 9 * v] = 0
        return {"base": base.reshape(-1)}
    case("air_check, base AIR of the memory table", "synchronises", ["bfs_air_check"], inputs, call, want,
         sensitive={"violations": np.arange(6, 16)})           # (first_row, count) of the five transition constraints that zero rows keep


_air_check()


# ------------------------------------------------------------------------------------------------ scans
def scan_parts(c, inp, v, n, k=0):
    kind, ncols, before, shift1 = [(0, 3, False, 0), (1, 2, False, 5)][(v + k) % 2]
    s = scalars(c, v, 10 + k, 3 * (1 + ncols) + 3)
    constants = [tuple(s[3 * j:3 * j + 3]) for j in range(1 + ncols)]
    initial = tuple(s[-3:])
    want = None
    if inp is not None:
        from stark_brainfuck_amd.table import Table
        cols = [inp["x%d_%d" % (j + 1, k)] for j in range(ncols)]
        if shift1:
            cols[0] = np.roll(cols[0], -shift1)
        want = Table.scan(kind, cols, inp["mask_%d" % k][:n].astype(bool), constants, initial, before)
    flat = [x for t in constants for x in t] + [0] * (12 - 3 * len(constants))
    return kind, ncols, before, shift1, (u64 * 12)(*flat), (u64 * 3)(*initial), want


def scan_inputs(c, v, n, k=0):
    rng = c.rng(v, 20 + k)
    inp = {"x%d_%d" % (j + 1, k): c.felt(v, 3 * k + j, n) for j in range(3)}
    inp["mask_%d" % k] = (rng.integers(0, 4, n) != 0).astype(np.uint8)
    return inp


def scan_case(n, host_terminal):
    stride = n + 5

    def call(lib, buf, stream, v):
        kind, ncols, before, shift1, constants, initial, _ = scan_parts(CASE, None, v, n)
        ptrs = [buf["x%d_0" % (j + 1)] if j < ncols else None for j in range(3)]
        terminal = (u64 * 3)() if host_terminal else None
        ck(lib, lib.bfs_xfe_scan_device(kind, ptrs[0], ptrs[1], ptrs[2], shift1, buf["mask_0"], n, constants, initial, int(before), buf["out"], stride,
                                        buf["terminal"], terminal, stream))
        if host_terminal:
            return {"host terminal": np.array(list(terminal), dtype=np.uint64)}

    def want(c, inp, v):
        states, terminal = scan_parts(c, inp, v, n)[6]
        out = {"out": strided(states, stride, np.zeros(3 * stride, dtype=np.uint64)), "terminal": np.array(terminal, dtype=np.uint64)}
        if host_terminal:
            out["host terminal"] = out["terminal"]
        return out
    CASE = case("xfe_scan_device n=%d%s" % (n, ", host terminal" if host_terminal else ""), "synchronises" if host_terminal else "enqueues",
                ["bfs_xfe_scan_device"], lambda c, v: scan_inputs(c, v, n), call, want, outputs={"out": 3 * stride, "terminal": 3},
                select={"out": rows_index(3, stride, n)}, sensitive={"out": rows_index(3, stride, n).reshape(3, n)[:, 16:].reshape(-1)})


scan_case(257, False)
scan_case(70001, False)
scan_case(257, True)


def _scan_many():
    sizes = [300, 4099]

    def call(lib, buf, stream, v):
        from stark_brainfuck_amd import _lib
        specs = []
        for k, n in enumerate(sizes):
            kind, ncols, before, shift1, constants, initial, _ = scan_parts(CASE, None, v, n, k)
            ptrs = [buf["x%d_%d" % (j + 1, k)] if j < ncols else None for j in range(3)]
            specs.append(_lib.ScanSpec(kind, int(before), ptrs[0], ptrs[1], ptrs[2], shift1, buf["mask_%d" % k], n, constants, initial, buf["out%d" % k],
                                       n + 5, buf["terminals"] + 64 * k))
        ck(lib, lib.bfs_xfe_scan_device_many((_lib.ScanSpec * len(specs))(*specs), len(specs), stream))

    def want(c, inp, v):
        out, terms = {}, np.zeros(8 * len(sizes), dtype=np.uint64)
        for k, n in enumerate(sizes):
            states, terminal = scan_parts(c, inp, v, n, k)[6]
            out["out%d" % k] = strided(states, n + 5, np.zeros(3 * (n + 5), dtype=np.uint64))
            terms[8 * k:8 * k + 3] = terminal
        out["terminals"] = terms
        return out

    def inputs(c, v):
        inp = {}
        for k, n in enumerate(sizes):
            inp.update(scan_inputs(c, v, n, k))
        return inp
    outputs = {"out%d" % k: 3 * (n + 5) for k, n in enumerate(sizes)}
    outputs["terminals"] = 8 * len(sizes)
    select = {"out%d" % k: rows_index(3, n + 5, n) for k, n in enumerate(sizes)}
    select["terminals"] = rows_index(len(sizes), 8, 3)
    sensitive = {"out%d" % k: rows_index(3, n + 5, n).reshape(3, n)[:, 16:].reshape(-1) for k, n in enumerate(sizes)}
    CASE = case("xfe_scan_device_many", "synchronises", ["bfs_xfe_scan_device_many"], inputs, call, want, outputs=outputs, select=select,
                sensitive=sensitive)


_scan_many()


# ------------------------------------------------------------------------------------------------ copies
def _copies():
    n = 5000
    case("memcpy_d2d", "enqueues", ["bfs_memcpy_d2d"], lambda c, v: {"in": c.felt(v, 0, n)},
         lambda lib, buf, stream, v: ck(lib, lib.bfs_memcpy_d2d(buf["out"], buf["in"], 8 * n, stream)),
         lambda c, inp, v: {"out": inp["in"]}, outputs={"out": n})
    case("memset", "enqueues", ["bfs_memset"], lambda c, v: {},
         lambda lib, buf, stream, v: ck(lib, lib.bfs_memset(buf["out"], 0x5A + v, 8 * n, stream)),
         lambda c, inp, v: {"out": np.full(n, (0x5A + v) * 0x0101010101010101, dtype=np.uint64)}, outputs={"out": n})
    sent = {}
    for label, words in (("small", 33), ("256 KiB + 8 from pageable memory", (256 << 10) // 8 + 1)):
        def h2d(lib, buf, stream, v, words=words, label=label):
            host = sent[label].felt(v, 5, words)             # pageable: a numpy array
            ck(lib, lib.bfs_memcpy_h2d(buf["out"], host.ctypes.data, 8 * words, stream))

        def d2h(lib, buf, stream, v, words=words):
            host = np.zeros(words, dtype=np.uint64)
            ck(lib, lib.bfs_memcpy_d2h(host.ctypes.data, buf["in"], 8 * words, stream))
            return {"host": host}
        sent[label] = case("memcpy_h2d, " + label, "synchronises", ["bfs_memcpy_h2d"], lambda c, v: {}, h2d,
                          lambda c, inp, v, words=words: {"out": c.felt(v, 5, words)}, outputs={"out": words})
        case("memcpy_d2h, " + label, "synchronises", ["bfs_memcpy_d2h"], lambda c, v, words=words: {"in": c.felt(v, 0, words)}, d2h,
             lambda c, inp, v: {"host": inp["in"]})


_copies()


# ------------------------------------------------------------------------------------------------ proof of work and FRI
def _pow():
    import fri_grinding_model as grinding
    bits = 10
    seed = lambda v: hashlib.sha256(b"stream order %d" % v).digest()

    def call(lib, buf, stream, v):
        nonce, found = u64(), ctypes.c_int()
        ck(lib, lib.bfs_pow_search(seed(v), bits, 0, 1 << 20, ctypes.byref(nonce), ctypes.byref(found), stream))
        return {"answer": np.array([found.value, nonce.value], dtype=np.uint64)}
    case("pow_search", "synchronises", ["bfs_pow_search"], lambda c, v: {}, call,
         lambda c, inp, v: {"answer": np.array([1, grinding.grind(seed(v), bits)], dtype=np.uint64)})


_pow()

FRI_LOG_N, FRI_EXPANSION, FRI_TESTS = 10, 4, 4


def serialized(lib, ps):
    length = ctypes.c_size_t()
    ck(lib, lib.bfs_ps_serialize(ps, 1 << 30, None, 0, ctypes.byref(length)))
    out = ctypes.create_string_buffer(length.value)
    ck(lib, lib.bfs_ps_serialize(ps, 1 << 30, out, length.value, ctypes.byref(length)))
    return out.raw[:length.value]


def fri_case(entry, a, coset_leaves, bits=0):
    import fri_folding_model as folding_model
    import fri_grinding_model as grinding
    n = 1 << FRI_LOG_N
    k = a.bit_length() - 1

    def inputs(c, v):
        o = oracle()
        return {"codeword": folding_model.codeword_of(o, c.base_seed + v, n, FRI_EXPANSION, OFFSET, o.primitive_nth_root(n)).reshape(-1)}

    def call(lib, buf, stream, v):
        omega = oracle().primitive_nth_root(n)
        ps = ctypes.c_void_p(lib.bfs_ps_new())
        indices = (u64 * FRI_TESTS)()
        try:
            if entry == "bfs_fri_prove":
                ck(lib, lib.bfs_fri_prove(ps, buf["codeword"], n, FRI_LOG_N, OFFSET, omega, FRI_EXPANSION, FRI_TESTS, indices, stream))
            elif entry == "bfs_fri_prove_folded":
                ck(lib, lib.bfs_fri_prove_folded(ps, buf["codeword"], n, FRI_LOG_N, OFFSET, omega, FRI_EXPANSION, k, FRI_TESTS, indices, stream))
            elif entry == "bfs_fri_prove_cosets":
                ck(lib, lib.bfs_fri_prove_cosets(ps, buf["codeword"], n, FRI_LOG_N, OFFSET, omega, FRI_EXPANSION, k, int(coset_leaves), FRI_TESTS, indices,
                                                 stream))
            else:
                session = ctypes.c_void_p(lib.bfs_fri_session_new())
                try:
                    ck(lib, lib.bfs_fri_session_set_folding(session, k))
                    ck(lib, lib.bfs_fri_session_set_coset_leaves(session, int(coset_leaves)))
                    ck(lib, lib.bfs_fri_session_set_grinding(session, bits, 0))
                    ck(lib, lib.bfs_fri_commit(session, ps, buf["codeword"], n, FRI_LOG_N, OFFSET, omega, FRI_EXPANSION, stream))
                    ck(lib, lib.bfs_fri_query(session, ps, FRI_TESTS, indices, stream))
                finally:
                    lib.bfs_fri_session_free(session)
            return {"transcript": digest_words(serialized(lib, ps)), "indices": np.array(list(indices), dtype=np.uint64)}
        finally:
            lib.bfs_ps_free(ps)

    def want(c, inp, v):
        o = oracle()
        ref = grinding.prove(o, inp["codeword"].reshape(3, n), OFFSET, o.primitive_nth_root(n), FRI_EXPANSION, FRI_TESTS, a, coset_leaves, bits)
        return {"transcript": digest_words(ref["proof_stream"].serialize()), "indices": np.array(ref["indices"], dtype=np.uint64)}
    entries = [entry] if entry != "commit + query" else ["bfs_fri_commit", "bfs_fri_query"]
    label = "%s: folding by %d%s%s" % (entry, a, ", coset leaves" if coset_leaves else "", ", grinding %d bits" % bits if bits else "")
    # the indices are a few small numbers drawn from the transcript: two inputs may share one, the transcript's digest tells them apart
    case(label, "synchronises", entries, inputs, call, want, sensitive={"indices": np.array([], dtype=np.int64)})


fri_case("bfs_fri_prove", 2, False)
fri_case("bfs_fri_prove_folded", 4, False)
fri_case("bfs_fri_prove_cosets", 2, False)
fri_case("bfs_fri_prove_cosets", 8, True)
fri_case("commit + query", 2, False, bits=6)


# ------------------------------------------------------------------------------------------------ what the table leaves out, and why
DEVICE_WIDE = {              # no `stream` parameter: documented device-wide waits and instruments, named here so that nobody looks for them
    "bfs_free": "bfs_free waits for the device",
    "bfs_pool_trim": "bfs_pool_trim returns the cached blocks to the driver",
    "bfs_event_elapsed_ms": "synchronises on `stop`",
    "bfs_ntt_route_forget": "which synchronises the device and frees what is no longer",
}
EXCLUDED = {
    "bfs_ntt_tune": "synchronises `stream` once, frees the buffers that lost",
    "bfs_event_record": "hipEvent-based timing on `stream`",
    "bfs_stark_commit": "Both synchronise `stream` several times",
    "bfs_stark_finish": "Both synchronise `stream` several times",
    "bfs_stark_push_openings": "One gather for everything; synchronises the stream.",
    "bfs_stark_push_openings_cosets": "rows, salts and row paths as above",
}
# the header gives these two no sentence: they are the instruments themselves -- the child waits for a stream with the one wherever a
# case needs a finished state, and tests/test_gpu_parity.py retires streams with the other (it synchronises the stream it destroys)
INSTRUMENTS = ("bfs_stream_synchronize", "bfs_stream_destroy")
# covered by the pool test of tests/stream_order_child.py, which is no case of this table
POOL_ENTRIES = ("bfs_malloc_async", "bfs_free_async")


def covered():
    return {e for c in CASES for e in c.entries} | set(POOL_ENTRIES)
