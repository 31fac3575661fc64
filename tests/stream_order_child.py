"""Child process of tests/test_gpu_stream_order.py: every case of tests/stream_cases.py through the C ABI on a held stream, in ONE
process that opens only the default stream, S (the stream under test) and T (the probe's), so that no other stream of the process can
share a hardware queue with the held one.  Prints one JSON line per control, case and pool test; a HIP error ends the run at once
with an "error" line and exit status 1.

    python tests/stream_order_child.py [--chain K] [--only SUBSTRING]

Per case: a warm run on S from a THIRD input (tables, scratch slots and pool blocks of these shapes exist afterwards, last released on
S, and what the library's scratch holds is no intermediate of the real input: a launch inside a chain that ran early or late reads
another input's leftovers, not stale right ones); the same run again between the legs; and
  leg 1  the operands hold a decoy; hold(S), the real inputs copied over the decoys and the flag are queued on S, the call is made on
         S, its outputs are copied to result buffers and read back on S.  The values must be the real inputs'; the flag must read 0 at
         the call's entry (and, for a call that only enqueues, at its return); the backlog's GPU time minus the host time from its
         first enqueue to the call's entry must be at least half of it.
  leg 2  hold(0) on the default stream; on S: real inputs in, the call, results out and back.  The values must be right, the flag must
         still read 0 (nothing in the call waited for the default stream or the device), and after the default stream has drained
         the outputs must read the same (nothing wrote them late).
A case whose hold ended early fails and says so."""
import ctypes
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (HERE, os.path.dirname(HERE)):
    if path not in sys.path:
        sys.path.insert(0, path)

import stream_cases as sc                      # noqa: E402
from stream_hold import ALL_ONES, CHAIN, Hold, HipError, ok   # noqa: E402


def emit(**line):
    print(json.dumps(line), flush=True)


class Runner:
    def __init__(self, lib, chain):
        self.lib = lib
        self.S, self.T = ctypes.c_void_p(), ctypes.c_void_p()
        ok(lib, lib.bfs_stream_create(ctypes.byref(self.S)))
        ok(lib, lib.bfs_stream_create(ctypes.byref(self.T)))
        self.hold = Hold(lib, self.T, chain)
        self.hold.warm(None)
        self.hold.warm(self.S)
        self.ev = [ctypes.c_void_p(), ctypes.c_void_p()]
        for e in self.ev:
            ok(lib, lib.bfs_event_create(ctypes.byref(e)))
        self.owned = []

    # ---- memory of a case: all of it from bfs_malloc, before any hold
    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        ok(self.lib, self.lib.bfs_malloc(ctypes.byref(p), max(nbytes, 8)), "bfs_malloc")
        self.owned.append(p)
        return p.value

    def release(self):
        for p in self.owned:
            ok(self.lib, self.lib.bfs_free(p), "bfs_free")
        self.owned = []

    def upload(self, ptr, words):
        ok(self.lib, self.lib.bfs_memcpy_h2d(ptr, words.ctypes.data, words.nbytes, self.S), "bfs_memcpy_h2d")

    def download(self, ptr, count):
        out = np.zeros(count, dtype=np.uint64)
        ok(self.lib, self.lib.bfs_memcpy_d2h(out.ctypes.data, ptr, 8 * count, self.S), "bfs_memcpy_d2h")
        return out

    def sync(self, stream):
        ok(self.lib, self.lib.bfs_stream_synchronize(stream), "bfs_stream_synchronize")

    words = staticmethod(sc.as_words)

    # ---- controls
    def control_streams_are_independent(self):
        """(a) with the default stream held, bfs_memset and bfs_memcpy_d2h on S return while the flag is 0"""
        scratch = self.alloc(64)
        self.hold.hold(None)
        ok(self.lib, self.lib.bfs_memset(scratch, 0x11, 64, self.S))
        got = self.download(scratch, 8)
        flag = self.hold.probe()
        self.sync(None)
        ms = self.hold.duration_ms()
        self.release()
        emit(control="a: S runs while the default stream is held", ok=bool(flag == 0 and (got == np.uint64(0x1111111111111111)).all()),
             flag=hex(flag), t_hold_ms=ms, enqueue_ms=1e3 * self.hold.enqueue_seconds, chain=self.hold.chain)
        return flag == 0

    def control_a_call_on_another_stream_is_seen(self):
        """(b) with S held and the real inputs queued behind the hold, bfs_gl_mul_pointwise made on T reads the decoys"""
        case = next(c for c in sc.CASES if c.name == "gl_mul_pointwise")
        real, decoy = case.inputs(0), case.inputs(sc.DECOY)
        want = case.want(real, 0)["out"]
        op = {k: self.alloc(a.nbytes) for k, a in real.items()}
        stage = {k: self.alloc(a.nbytes) for k, a in real.items()}
        out = self.alloc(8 * want.size)
        for k in real:
            self.upload(op[k], decoy[k])
            self.upload(stage[k], real[k])
        ok(self.lib, self.lib.bfs_memset(out, 0, 8 * want.size, self.S))
        self.sync(self.S)
        self.hold.hold(self.S, then=lambda: [ok(self.lib, self.lib.bfs_memcpy_d2d(op[k], stage[k], real[k].nbytes, self.S)) for k in real])
        case.call(self.lib, dict(op, out=out), self.T, 0)
        got = np.zeros(want.size, dtype=np.uint64)
        ok(self.lib, self.lib.bfs_memcpy_d2h(got.ctypes.data, out, got.nbytes, self.T))
        flag = self.hold.probe()
        self.sync(self.S)
        self.release()
        emit(control="b: a call made on T instead of S computes from the decoy", ok=bool(flag == 0 and (got != want).any()), flag=hex(flag),
             words_that_differ=int((got != want).sum()), words=int(want.size))

    # ---- one case
    def run_case(self, case):
        lib, S, hold = self.lib, self.S, self.hold
        variants = case.variants
        real = {v: case.inputs(v) for v in variants}
        decoy = {k: self.words(a) for k, a in case.inputs(sc.DECOY).items()}
        want = {v: case.want(real[v], v) for v in variants}
        other = {k: self.words(a) for k, a in case.inputs(sc.WARM).items()}
        want_other = {v: case.want(case.inputs(sc.WARM), v) for v in variants}
        fixed = {k: self.words(a) for k, a in case.fixed().items()}
        fix = {k: self.alloc(a.nbytes) for k, a in fixed.items()}
        for k, a in fixed.items():
            self.upload(fix[k], a)
        op, stage, out, res = {}, {}, {}, {}
        for v in variants:
            real[v] = {k: self.words(a) for k, a in real[v].items()}
            op[v] = {k: self.alloc(a.nbytes) for k, a in real[v].items()}
            stage[v] = {k: self.alloc(a.nbytes) for k, a in real[v].items()}
            for k, a in real[v].items():
                self.upload(stage[v][k], a)
            out[v] = {k: self.alloc(8 * n) for k, n in case.outputs.items() if k not in real[v]}
            res[v] = {k: self.alloc(8 * n) for k, n in case.outputs.items()}
        where = {v: dict(fix, **op[v], **out[v]) for v in variants}
        failures, figures = [], {}

        def reset():
            for v in variants:
                for k, a in decoy.items():
                    self.upload(op[v][k], a)
                for k, n in case.outputs.items():
                    if k in out[v]:
                        ok(lib, lib.bfs_memset(out[v][k], 0, 8 * n, S))
                    ok(lib, lib.bfs_memset(res[v][k], 0, 8 * n, S))
            self.sync(S)

        def real_inputs_in():
            for v in variants:
                for k, a in real[v].items():
                    ok(lib, lib.bfs_memcpy_d2d(op[v][k], stage[v][k], a.nbytes, S), "bfs_memcpy_d2d")

        def calls():
            return {v: case.call(lib, where[v], S, v) or {} for v in variants}

        def results_out():
            for v in variants:
                for k, n in case.outputs.items():
                    ok(lib, lib.bfs_memcpy_d2d(res[v][k], where[v][k], 8 * n, S), "bfs_memcpy_d2d")

        def read_back():
            return {v: {k: self.download(res[v][k], n) for k, n in case.outputs.items()} for v in variants}

        def compare(leg, device, host, want=want):
            for v in variants:
                got = dict(device[v])
                for k, a in host[v].items():
                    got[k] = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
                for k, w in want[v].items():
                    if k not in got or got[k].size != w.size:
                        failures.append("%s: call %d has no result %r of %d words" % (leg, v, k, w.size))
                        continue
                    select = case.selected(k, w.size)
                    wrong = np.flatnonzero(got[k][select] != w[select])
                    if wrong.size:
                        at = int(select[wrong[0]])
                        failures.append("%s: call %d, %s: %d of %d words differ from the reference, first at %d: %x, expected %x" % (
                            leg, v, k, wrong.size, select.size, at, int(got[k][at]), int(w[at])))
                    if k in out[v]:
                        rest = np.ones(w.size, dtype=bool)
                        rest[select] = False
                        if got[k][rest].any():
                            failures.append("%s: call %d, %s: %d words outside the result were written" % (leg, v, k, int((got[k][rest] != 0).sum())))

        def run_on_the_third_input(label):
            """the same shapes on S from the WARM input, checked against its own reference: tables, scratch slots and pool blocks of these
            shapes exist afterwards, last released on S, and every intermediate the library keeps is another input's"""
            reset()
            for v in variants:
                for k, a in other.items():
                    self.upload(op[v][k], a)
            host = calls()
            results_out()
            compare(label, read_back(), host, want_other)

        run_on_the_third_input("warm run")

        # leg 1: order behind the caller's own stream
        reset()
        t0 = hold.hold(S, then=real_inputs_in)
        at_entry = hold.probe()
        entry = time.perf_counter()
        host = calls()
        at_return = hold.probe()
        returned = time.perf_counter()
        results_out()
        device = read_back()
        t_hold = hold.duration_ms()
        lead = 1e3 * (entry - t0)
        figures.update(t_hold_ms=round(t_hold, 3), lead_ms=round(lead, 3), call_ms=round(1e3 * (returned - entry), 3))
        if at_entry != 0:
            failures.append("leg 1: the hold ended before the call was made (flag %x at entry)" % at_entry)
        if t_hold - lead < t_hold / 2:
            failures.append("leg 1: the hold ended early: %.2f ms of backlog, %.2f ms gone before the call's entry" % (t_hold, lead))
        if case.kind == "enqueues" and at_return != 0:
            failures.append("leg 1: the call does not only enqueue: the flag read %x when it returned" % at_return)
        compare("leg 1", device, host)

        # leg 2: nothing leaks to the default stream, nothing waits for it
        run_on_the_third_input("run between the legs")
        reset()
        hold.hold(None)
        ok(lib, lib.bfs_event_record(self.ev[0], S))
        real_inputs_in()
        host = calls()
        results_out()
        ok(lib, lib.bfs_event_record(self.ev[1], S))
        device = read_back()
        flag = hold.probe()
        compare("leg 2", device, host)
        if flag != 0:
            failures.append("leg 2: the hold on the default stream ended before the case did, or the call waited for it (flag %x)" % flag)
        self.sync(None)
        results_out()
        late = read_back()
        for v in variants:
            for k in device[v]:
                if not np.array_equal(device[v][k], late[v][k]):
                    failures.append("leg 2: call %d, %s changed after the default stream drained: written late" % (v, k))
        ms = ctypes.c_float()
        ok(lib, lib.bfs_event_elapsed_ms(self.ev[0], self.ev[1], ctypes.byref(ms)))
        figures.update(held_case_ms=round(float(ms.value), 3), t_hold0_ms=round(hold.duration_ms(), 3))
        self.sync(S)
        self.release()
        emit(case=case.name, kind=case.kind, ok=not failures, failures=failures, **figures)

    # ---- the pool
    def pool(self):
        lib, S, T, hold = self.lib, self.S, self.T, self.hold
        size, words = 5 << 20, (5 << 20) // 8                 # a size class of its own: nothing else here allocates 5 MiB
        pattern = sc.oracle().felt_array(sc.SEED, 0, words)
        for label, second in (("another stream", T), ("the same stream", S)):
            self.sync(None), self.sync(S), self.sync(T)
            ok(lib, lib.bfs_pool_trim(), "bfs_pool_trim")
            result = self.alloc(size + (1 << 20))
            b = ctypes.c_void_p()
            ok(lib, lib.bfs_malloc_async(ctypes.byref(b), size, S), "bfs_malloc_async")
            self.upload(b, pattern)
            hold.hold(S, then=lambda: ok(lib, lib.bfs_memcpy_d2d(result, b, size, S)))
            ok(lib, lib.bfs_free_async(b, S), "bfs_free_async")
            again = ctypes.c_void_p()
            ok(lib, lib.bfs_malloc_async(ctypes.byref(again), size, second), "bfs_malloc_async")
            flag = hold.probe()
            ok(lib, lib.bfs_memset(again, 0, size, second))
            self.sync(second)
            got = self.download(result, words)
            failures = []
            if again.value != b.value:
                failures.append("bfs_malloc_async did not hand the released block out again: the case shows nothing")
            if second is S and flag != 0:
                failures.append("a request on the releasing stream waited (flag %x)" % flag)
            if second is T and flag != ALL_ONES:
                failures.append("a request on another stream came back while the releasing stream still held work on the block")
            if not np.array_equal(got, pattern):
                failures.append("%d words of the copy queued before the release are not the block's" % int((got != pattern).sum()))
            self.sync(S)
            ok(lib, lib.bfs_free_async(again, second), "bfs_free_async")
            self.sync(second)
            self.release()
            emit(pool="released on S, requested on " + label, ok=not failures, failures=failures)


def main(argv):
    chain = int(argv[argv.index("--chain") + 1]) if "--chain" in argv else CHAIN
    only = argv[argv.index("--only") + 1] if "--only" in argv else None
    from stark_brainfuck_amd import _lib
    lib = _lib.load()
    try:
        run = Runner(lib, chain)
        independent = run.control_streams_are_independent()
        run.control_a_call_on_another_stream_is_seen()
        if not independent:
            emit(error="the streams of this process are not independent: leg 2 cannot be judged")
            return 1
        for case in sc.CASES:
            if only is None or only in case.name:
                run.run_case(case)
        if only is None:
            run.pool()
        emit(done=True)
        return 0
    except (HipError, RuntimeError) as e:
        emit(error=str(e))
        return 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
