"""A painted arena and its checker: what a kernel does to memory that is NOT its result.

One allocation holds a front guard, the payload and a back guard.  The payload is `batch` rows `stride` units apart of which the
first `n` are result (or any list of result ranges); the call under test gets the payload's address.  Everything is painted before
the call and compared with a snapshot taken afterwards:
  * uint64 arenas are painted 0xFFFFFFFFDEADBEEF, which is >= p = 2^64 - 2^32 + 1: no correct kernel produces it as a residue;
  * byte arenas (Merkle nodes, scan masks) are painted 0xA5;
  * a guard is 4096 words, the largest footprint one workgroup has anywhere in the library (4096-element NTT tiles, 2048-element
    batch-inverse groups); gaps inside a batch are the caller's choice, small and odd.
The checker works on numpy snapshots alone (Layout, first_change): tests/test_painted_arena_host.py checks it without a GPU.  Arena
puts a Layout into a DeviceBuffer.  In production the neighbour of an output is a live buffer of the same proof (every buffer comes
from the library's pool), so a stray store does not fault: it corrupts."""
import numpy as np

PAINT_WORD = 0xFFFFFFFFDEADBEEF
PAINT_BYTE = 0xA5
GUARD_WORDS = 4096
P = (1 << 64) - (1 << 32) + 1
assert PAINT_WORD >= P


class Violation(AssertionError):
    """a changed unit outside the result ranges, or a changed input.  region: "front guard", "gap b", "back guard" or the name of
    an input; offset: units from the start of that region; index: units from the start of the snapshot."""

    def __init__(self, region, offset, index, before, after):
        self.region, self.offset, self.index, self.before, self.after = region, int(offset), int(index), int(before), int(after)
        AssertionError.__init__(self, "%s, offset %d (unit %d of the buffer): 0x%X became 0x%X" % (region, offset, index, before, after))


def first_change(before, after):
    """index of the first unit that differs between two snapshots, None if there is none"""
    before, after = np.asarray(before).reshape(-1), np.asarray(after).reshape(-1)
    assert before.shape == after.shape and before.dtype == after.dtype
    changed = np.flatnonzero(before != after)
    return int(changed[0]) if changed.size else None


class Layout:
    """geometry of an arena in units of its dtype (uint64 words or bytes).  results: (offset, length) ranges relative to the payload,
    ascending and disjoint; the default is `batch` rows of `n` units, `stride` apart.  The payload is batch * stride units unless
    `payload` says otherwise.  Regions outside the results, in address order: "front guard", "head gap" (payload in front of the
    first result, if any), "gap 0", "gap 1", ..., "back guard": gap b is what follows result b -- with the default ranges units
    n .. stride of row b."""

    def __init__(self, batch=1, stride=None, n=None, dtype=np.uint64, results=None, payload=None, guard=None):
        self.dtype = np.dtype(dtype)
        assert self.dtype in (np.dtype(np.uint64), np.dtype(np.uint8))
        self.paint = PAINT_WORD if self.dtype == np.dtype(np.uint64) else PAINT_BYTE
        self.guard = (GUARD_WORDS * 8 // self.dtype.itemsize) if guard is None else int(guard)
        if results is None:
            stride = n if stride is None else stride
            assert stride >= n
            results = [(b * stride, n) for b in range(batch)]
            payload = batch * stride if payload is None else payload
        self.batch, self.stride, self.n = batch, stride, n
        self.results = [(int(o), int(l)) for o, l in results if l > 0]
        self.payload = int(payload)
        end = 0
        for o, l in self.results:
            assert o >= end, "result ranges must be ascending and disjoint"
            end = o + l
        assert end <= self.payload
        self.total = -(-(2 * self.guard + self.payload) * self.dtype.itemsize // 8) * 8 // self.dtype.itemsize     # whole words
        # the complement of the results, as (name, start, stop) in units from the start of the arena
        self.regions = [("front guard", 0, self.guard)]
        at, name = self.guard, "head gap"
        for k, (o, l) in enumerate(self.results):
            if self.guard + o > at:
                self.regions.append((name, at, self.guard + o))
            at, name = self.guard + o + l, "gap %d" % k
        if self.guard + self.payload > at:
            self.regions.append((name, at, self.guard + self.payload))
        self.regions.append(("back guard", self.guard + self.payload, self.total))

    def painted(self):
        """the arena before anything is written: all paint"""
        return np.full(self.total, self.paint, dtype=self.dtype)

    def payload_of(self, snapshot):
        return snapshot[self.guard:self.guard + self.payload]

    def result(self, snapshot, k=0):
        o, l = self.results[k]
        return snapshot[self.guard + o:self.guard + o + l]

    def rows(self, snapshot):
        """the default layout's results as a (batch, n) array"""
        return np.stack([self.result(snapshot, b) for b in range(len(self.results))])

    def violation(self, before, after):
        """the first changed unit outside the result ranges as a Violation, None when there is none.  What a result range holds is
        not looked at: a result that contains the paint value is no violation."""
        before, after = np.asarray(before).reshape(-1), np.asarray(after).reshape(-1)
        assert before.shape == after.shape == (self.total,)
        for name, start, stop in self.regions:
            k = first_change(before[start:stop], after[start:stop])
            if k is not None:
                return Violation(name, k, start + k, before[start + k], after[start + k])
        return None

    def check(self, before, after, inputs=()):
        """raises the Violation of the first stray write, or of the first changed unit of an input: inputs = (name, before, after)
        snapshots"""
        v = self.violation(before, after)
        if v is None:
            v = input_violation(inputs)
        if v is not None:
            raise v


def input_violation(inputs):
    """inputs: (name, before, after) snapshot triples; the first changed unit of the first changed input as a Violation, or None"""
    for name, before, after in inputs:
        k = first_change(before, after)
        if k is not None:
            b, a = np.asarray(before).reshape(-1), np.asarray(after).reshape(-1)
            return Violation("input %s" % name, k, k, b[k], a[k])
    return None


class Arena:
    """a Layout in HBM: one DeviceBuffer, painted; `ptr` is the payload's address (16-byte aligned).  fill() puts data into the
    payload (an in-place call's operand), snapshot() reads the whole allocation back."""

    def __init__(self, layout=None, **kw):
        from stark_brainfuck_amd.device import DeviceBuffer
        self.layout = layout if layout is not None else Layout(**kw)
        self.itemsize = self.layout.dtype.itemsize
        self.image = self.layout.painted()           # host copy of what was uploaded: the snapshot before the call
        self.buf = DeviceBuffer.from_numpy(self.image.view(np.uint64))
        self.ptr = self.buf.ptr + self.layout.guard * self.itemsize
        assert self.ptr % 16 == 0

    @property
    def nbytes(self):
        return self.buf.nbytes

    def address(self, offset):
        """device address of payload unit `offset`"""
        return self.ptr + int(offset) * self.itemsize

    def fill(self, offset, values):
        from stark_brainfuck_amd import _lib
        from stark_brainfuck_amd.device import current_stream, synchronize
        values = np.ascontiguousarray(values, dtype=self.layout.dtype).reshape(-1)
        assert 0 <= offset and offset + values.size <= self.layout.payload
        if values.size:
            g = self.layout.guard
            self.image[g + offset:g + offset + values.size] = values
            _lib.check(_lib.load().bfs_memcpy_h2d(self.address(offset), values.ctypes.data, values.nbytes, current_stream()))
            synchronize()

    def fill_rows(self, rows):
        """row b of a (batch, k) array to payload offset b * stride"""
        for b, row in enumerate(rows):
            self.fill(b * self.layout.stride, row)

    def snapshot(self):
        from stark_brainfuck_amd.device import synchronize
        synchronize()
        return self.buf.to_numpy().view(self.layout.dtype)[:self.layout.total].copy()

    def rows(self, snapshot):
        return self.layout.rows(snapshot)

    def check(self, before, after, inputs=()):
        self.layout.check(before, after, inputs)

    def contained(self, inputs=()):
        """after the call under test: a snapshot checked against the image that went up (and the inputs' snapshots); returns it"""
        after = self.snapshot()
        self.layout.check(self.image, after, inputs)
        return after
