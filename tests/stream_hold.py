"""Holding a stream busy with the library's own asynchronous calls, for tests/stream_order_child.py.

hold(stream) enqueues a finite backlog on `stream`: CHAIN out-of-place bfs_gl_ntt calls of 2^24 points (128 MiB each way, below the
256 MiB from which bfs_ntt_tune's routes matter) that ping-pong between two buffers, with a bfs_event_record in front and behind; then
a small bfs_memcpy_d2d between the two buffers, whatever the caller wants ordered behind the backlog (`then`), and last a bfs_memset
that turns the 8-byte flag word in HBM from 0 into all-ones.  Nothing spins and nothing waits on a condition: the backlog ends by
itself.  probe() reads the flag with bfs_memcpy_d2h on a third stream, which synchronises that stream only.

CHAIN comes from profiles/stream_order.md: at least four times the longest held case, measured with bfs_event_elapsed_ms."""
import ctypes
import time

HOLD_LOG_N = 24
CHAIN = 512
ALL_ONES = (1 << 64) - 1


class HipError(RuntimeError):
    pass


def ok(lib, rc, what=""):
    if rc != 0:
        raise HipError("%s: error %d: %s" % (what or "call", rc, lib.bfs_last_error().decode("utf-8", "replace")))


class Hold:
    def __init__(self, lib, probe_stream, chain=CHAIN):
        self.lib, self.T, self.chain = lib, probe_stream, chain
        self.n = 1 << HOLD_LOG_N
        self.root = lib.bfs_gl_primitive_root(HOLD_LOG_N)
        self.a, self.b, self.flag, self.h_flag = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        for ptr, size in ((self.a, 8 * self.n), (self.b, 8 * self.n), (self.flag, 256)):
            ok(lib, lib.bfs_malloc(ctypes.byref(ptr), size), "bfs_malloc")
        ok(lib, lib.bfs_host_alloc(ctypes.byref(self.h_flag), 8), "bfs_host_alloc")
        self.start, self.stop = ctypes.c_void_p(), ctypes.c_void_p()
        ok(lib, lib.bfs_event_create(ctypes.byref(self.start)))
        ok(lib, lib.bfs_event_create(ctypes.byref(self.stop)))
        ok(lib, lib.bfs_memset(self.a, 0, 8 * self.n, None))            # zeros are canonical residues, and stay zeros
        ok(lib, lib.bfs_memset(self.b, 0, 8 * self.n, None))
        ok(lib, lib.bfs_stream_synchronize(None))
        self.enqueued_at = None

    def warm(self, stream):
        """one transform each way on `stream`, finished: the tables of this shape exist afterwards"""
        self._ntt(self.a, self.b, stream)
        self._ntt(self.b, self.a, stream)
        ok(self.lib, self.lib.bfs_stream_synchronize(stream))

    def _ntt(self, src, dst, stream):
        ok(self.lib, self.lib.bfs_gl_ntt(src, self.n, self.n, dst, self.n, HOLD_LOG_N, 1, self.root, 1, 1, stream), "bfs_gl_ntt (hold)")

    def clear(self):
        """flag := 0, finished, before a hold is enqueued"""
        ok(self.lib, self.lib.bfs_memset(self.flag, 0, 8, self.T))
        ok(self.lib, self.lib.bfs_stream_synchronize(self.T))

    def hold(self, stream, then=None):
        """-> the host time just before the first call of the backlog"""
        lib = self.lib
        self.clear()
        self.enqueued_at = time.perf_counter()
        ok(lib, lib.bfs_event_record(self.start, stream))
        for k in range(self.chain):
            self._ntt(self.a, self.b, stream) if k % 2 == 0 else self._ntt(self.b, self.a, stream)
        ok(lib, lib.bfs_event_record(self.stop, stream))
        self.enqueue_seconds = time.perf_counter() - self.enqueued_at
        ok(lib, lib.bfs_memcpy_d2d(self.b, self.a, 4096, stream))
        if then is not None:
            then()
        ok(lib, lib.bfs_memset(self.flag, 0xFF, 8, stream))
        return self.enqueued_at

    def probe(self):
        """the flag word now: 0 while the backlog runs, all-ones once the stream got past it"""
        ok(self.lib, self.lib.bfs_memcpy_d2h(self.h_flag, self.flag, 8, self.T), "bfs_memcpy_d2h (probe)")
        return ctypes.c_uint64.from_address(self.h_flag.value).value

    def duration_ms(self):
        """GPU time of the last backlog (waits for its end)"""
        ms = ctypes.c_float()
        ok(self.lib, self.lib.bfs_event_elapsed_ms(self.start, self.stop, ctypes.byref(ms)))
        return float(ms.value)
