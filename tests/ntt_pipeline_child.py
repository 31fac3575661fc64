"""The child process of tests/test_gpu_ntt_pipeline.py: BFS_NTT_PIPELINE is read once per process, so every route gets a process of
its own.  `python ntt_pipeline_child.py cases` runs the transform cases and prints one JSON line per case -- the sha256 of every
output column, whether it equals the oracle's, whether the words between the columns kept their fill; `... order` runs the stream
order, capture and thread cases (forced route only).  Before each case the child writes "case NAME" to stderr, where the library's
BFS_NTT_PLAN_LOG lines go, so that the parent can tell which route each call took."""
import ctypes
import hashlib
import json
import os
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from oracle import ref_oracle as o                    # noqa: E402
from stark_brainfuck_amd import _lib                  # noqa: E402

P = (1 << 64) - (1 << 32) + 1
SEED = 0x9199E
FILL = 0xA5                                           # bytes of an output buffer before the call
FILL_WORD = int.from_bytes(bytes([FILL]) * 8, "little")
lib = _lib.load()


def mark(name):
    os.write(2, ("case %s\n" % name).encode())


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<u8").tobytes()).hexdigest()


def edge_column(n, seed):
    """values next to 0, next to p and around 2^32 with a few random ones (the generator of tests/test_gpu_parity.py: edge_values)"""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 6, n, dtype=np.uint64)
    kind = rng.integers(0, 8, n)
    v = np.where(kind < 3, small, np.uint64(P) - np.uint64(1) - small)
    v = np.where(kind == 6, rng.integers(0, P, n, dtype=np.uint64), v)
    v = np.where(kind == 7, (np.uint64(1) << np.uint64(32)) - small, v)
    return np.ascontiguousarray(v, dtype=np.uint64)


def columns(n, batch, tag):
    """`batch` columns: splitmix, edge values, all p - 1, alternating 1 / p - 1, then splitmix again"""
    kinds = [lambda c: o.felt_array(SEED + tag + (c << 32), 0, n), lambda c: edge_column(n, SEED + tag + c),
             lambda c: np.full(n, P - 1, dtype=np.uint64), lambda c: np.where(np.arange(n) % 2 == 0, np.uint64(1), np.uint64(P - 1)).astype(np.uint64)]
    if batch == 2:                                    # the two that drive the butterfly sums over p
        kinds = [kinds[1], kinds[3]]
    return [np.ascontiguousarray(kinds[c % len(kinds)](c), dtype=np.uint64) for c in range(batch)]


class Buf:
    """plain bfs_malloc memory (no pool: these buffers are used from several streams)"""

    def __init__(self, words, fill=None):
        self.words, self.p = words, ctypes.c_void_p()
        _lib.check(lib.bfs_malloc(ctypes.byref(self.p), 8 * words))
        if fill is not None:
            _lib.check(lib.bfs_memset(self.p, fill, 8 * words, None))
            _lib.check(lib.bfs_stream_synchronize(None))

    @property
    def ptr(self):
        return self.p.value

    def put(self, a, offset=0):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        _lib.check(lib.bfs_memcpy_h2d(self.ptr + 8 * offset, a.ctypes.data, a.nbytes, None))

    def get(self, stream=None):
        out = np.empty(self.words, dtype=np.uint64)
        _lib.check(lib.bfs_memcpy_d2h(out.ctypes.data, self.ptr, 8 * self.words, stream))
        return out

    def free(self):
        _lib.check(lib.bfs_free(self.p))


def ntt(din, n_in, in_stride, dout, out_stride, logn, batch, root, shift=1, scale=1, stream=None):
    _lib.check(lib.bfs_gl_ntt(din, n_in, in_stride, dout, out_stride, logn, batch, root, shift, scale, stream))


def run_case(name, logn, batch, in_stride=None, out_stride=None, inverse=False, shift=1, n_in=None, in_place=False):
    n = 1 << logn
    n_in = n if n_in is None else n_in
    in_stride = n_in if in_stride is None else in_stride
    out_stride = n if out_stride is None else out_stride
    w = o.primitive_nth_root(n)
    cols = [c[:n_in] for c in columns(n, batch, logn * 131 + batch)]
    if inverse:
        want = [o.intt(w, c) for c in cols]
        root, scale = o.inv(w), o.inv(n)
    elif n_in < n or shift != 1:
        want = [o.fast_coset_evaluate(c, shift, w, n) for c in cols]
        root, scale = w, 1
    else:
        want = [o.ntt(w, c) for c in cols]
        root, scale = w, 1
    if in_place:
        assert in_stride == out_stride and n_in == n
        dout = din = Buf(batch * out_stride, FILL)
    else:
        din, dout = Buf(batch * in_stride, 0), Buf(batch * out_stride, FILL)
    for c, col in enumerate(cols):
        din.put(col, c * in_stride)
    mark(name)
    ntt(din.ptr, n_in, in_stride, dout.ptr, out_stride, logn, batch, root, shift, scale)
    _lib.check(lib.bfs_stream_synchronize(None))
    got = dout.get()
    kept_in = in_place or all((din.get()[c * in_stride:c * in_stride + n_in] == col).all() for c, col in enumerate(cols))
    gaps = all((got[c * out_stride + n:(c + 1) * out_stride] == FILL_WORD).all() for c in range(batch))
    print(json.dumps({"case": name, "sha": [sha(got[c * out_stride:c * out_stride + n]) for c in range(batch)],
                      "oracle": [bool((got[c * out_stride:c * out_stride + n] == want[c]).all()) for c in range(batch)],
                      "gaps_kept": bool(gaps), "input_kept": bool(kept_in)}), flush=True)
    dout.free()
    if not in_place:
        din.free()


def cases():
    for batch in (2, 3, 5):
        run_case("three_pass_b%d" % batch, 17, batch)
    run_case("two_pass_b2", 13, 2)
    run_case("strides", 17, 3, in_stride=(1 << 17) + 8, out_stride=(1 << 17) + 40)
    run_case("inverse", 17, 3, inverse=True)
    run_case("coset_quarter", 17, 2, shift=7, n_in=1 << 15)
    run_case("in_place", 17, 2, in_place=True)


# ------------------------------------------------------------------------------------------------ order, capture, threads
def stream_order():
    """A forced-route call behind a backlog on its own stream: while the backlog runs, none of its launches has run on either stream
    (the output still holds its fill); a copy enqueued on that stream right after the call reads every column finished."""
    from stream_hold import Hold
    logn, batch = 17, 5
    n = 1 << logn
    w = o.primitive_nth_root(n)
    cols = columns(n, batch, 7)
    want = np.concatenate([o.ntt(w, c) for c in cols])
    S, T = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(lib.bfs_stream_create(ctypes.byref(S)))
    _lib.check(lib.bfs_stream_create(ctypes.byref(T)))
    din, dout, snap = Buf(batch * n, 0), Buf(batch * n, FILL), Buf(batch * n, 0)
    din.put(np.concatenate(cols))
    hold = Hold(lib, T)
    hold.warm(S)
    mark("order_warm")
    ntt(din.ptr, n, n, dout.ptr, n, logn, batch, w, stream=S)         # tables and the second stream exist from here on
    _lib.check(lib.bfs_stream_synchronize(S))
    warm_ok = bool((dout.get(T) == want).all())
    _lib.check(lib.bfs_memset(dout.p, FILL, 8 * batch * n, S))
    _lib.check(lib.bfs_stream_synchronize(S))

    def then():
        mark("order_held")
        ntt(din.ptr, n, n, dout.ptr, n, logn, batch, w, stream=S)
        _lib.check(lib.bfs_memcpy_d2d(snap.p, dout.p, 8 * batch * n, S))
    hold.hold(S, then)
    flag_before = hold.probe()
    during = dout.get(T)
    flag_after = hold.probe()
    _lib.check(lib.bfs_stream_synchronize(S))
    print(json.dumps({"case": "stream_order", "warm_ok": warm_ok, "held_before_read": flag_before == 0, "held_after_read": flag_after == 0,
                      "untouched_while_held": bool((during == FILL_WORD).all()), "words_written_while_held": int((during != FILL_WORD).sum()),
                      "copy_after_call_sees_all": bool((snap.get() == want).all()), "flag_at_end": hold.probe() == (1 << 64) - 1,
                      "backlog_ms": hold.duration_ms()}), flush=True)
    _lib.check(lib.bfs_stream_destroy(S))
    _lib.check(lib.bfs_stream_destroy(T))


def capture():
    """A call captured into a graph takes one launch per pass (the second stream is not part of the caller's graph) and replays to
    the oracle's bytes."""
    import torch
    logn, batch = 17, 3
    n = 1 << logn
    w = o.primitive_nth_root(n)
    cols = columns(n, batch, 11)
    want = np.concatenate([o.ntt(w, c) for c in cols])
    din, dout = Buf(batch * n, 0), Buf(batch * n, FILL)
    din.put(np.concatenate(cols))
    s = torch.cuda.Stream()
    mark("capture_warm")
    ntt(din.ptr, n, n, dout.ptr, n, logn, batch, w, stream=s.cuda_stream)
    s.synchronize()
    eager = dout.get()
    _lib.check(lib.bfs_memset(dout.p, FILL, 8 * batch * n, None))
    _lib.check(lib.bfs_stream_synchronize(None))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        mark("capture_capturing")
        ntt(din.ptr, n, n, dout.ptr, n, logn, batch, w, stream=torch.cuda.current_stream().cuda_stream)
    mark("capture_done")
    torch.cuda.synchronize()
    not_run_by_capture = bool((dout.get() == FILL_WORD).all())
    replays = []
    for _ in range(2):
        _lib.check(lib.bfs_memset(dout.p, FILL, 8 * batch * n, None))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        replays.append(bool((dout.get() == want).all()))
    print(json.dumps({"case": "capture", "eager_ok": bool((eager == want).all()), "capture_ran_nothing": not_run_by_capture, "replays_ok": replays}), flush=True)


def threads():
    """two host threads, a stream each, forced-route calls at 2^17: the oracle's bytes in both"""
    logn, batch, reps = 17, 3, 6
    n = 1 << logn
    w = o.primitive_nth_root(n)
    results = [None, None]
    work = []
    for t in range(2):
        cols = columns(n, batch, 100 + t)
        S = ctypes.c_void_p()
        _lib.check(lib.bfs_stream_create(ctypes.byref(S)))
        din, dout = Buf(batch * n, 0), Buf(batch * n, FILL)
        din.put(np.concatenate(cols))
        work.append((S, din, dout, np.concatenate([o.ntt(w, c) for c in cols])))
    mark("threads_warm")
    ntt(work[0][1].ptr, n, n, work[0][2].ptr, n, logn, batch, w)          # the tables exist before the threads start
    _lib.check(lib.bfs_stream_synchronize(None))
    mark("threads")

    def body(t):
        S, din, dout, want = work[t]
        good = []
        try:
            for _ in range(reps):
                _lib.check(lib.bfs_memset(dout.p, FILL, 8 * batch * n, S))
                ntt(din.ptr, n, n, dout.ptr, n, logn, batch, w, stream=S)
                good.append(bool((dout.get(S) == want).all()))
            results[t] = good
        except Exception as e:                                           # noqa: BLE001
            results[t] = repr(e)
    ts = [threading.Thread(target=body, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    print(json.dumps({"case": "threads", "results": results}), flush=True)
    for S, _, _, _ in work:
        _lib.check(lib.bfs_stream_destroy(S))


if __name__ == "__main__":
    try:
        if sys.argv[1] == "cases":
            cases()
        else:
            stream_order()
            threads()
            capture()
        print(json.dumps({"done": True}), flush=True)
    except Exception as e:                                               # noqa: BLE001
        print(json.dumps({"error": repr(e)}), flush=True)
        raise
