#!/usr/bin/env python3
"""Times bfs_air_check on the processor table at 2^18, 2^20, 2^22 and 2^24 rows, base and full mode, end to end (the call is synchronous:
output reset, launch, read-back of the result).  The trace is a real one -- a nested-loop program, padded and extended, 2^18 rows --
repeated in HBM to the larger sizes, so that almost every row satisfies the AIR as in a real check (the seams between the copies
fail a few transition constraints; their counts are printed).

    python tools/air_check_time.py [--reps 20]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--logs", default="18,20,22,24")
    args = ap.parse_args()
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    from stark_brainfuck_amd.device import DeviceBuffer, current_stream
    from stark_brainfuck_amd.vm import VirtualMachine
    lib, stream = _lib.load(), current_stream()
    u64 = ctypes.c_uint64
    code = "+" * 128 + "[>" + "+" * 128 + "[>++++<-]<-]+++."
    program = VirtualMachine.compile(code)
    matrices = VirtualMachine.simulate(program, input_data=[], max_cycles=1 << 22)
    stark = BrainfuckStark(len(matrices[0]), len(matrices[1]), program, [], [chr(int(v) % 256) for v in matrices[4].values.reshape(-1)])
    t = stark.processor_table
    t.matrix = matrices[0]
    t.pad()
    challenges = [((7 * i + 3) << 40 | 12345, (i + 1) << 35, 99 + i) for i in range(11)]
    initials = [(1 << 50 | 77, 5, 6), (3 << 45 | 11, 7, 8)]
    t.extend(challenges, initials)
    terminals = [t.instruction_permutation_terminal, t.memory_permutation_terminal, t.input_evaluation_terminal,
                 t.output_evaluation_terminal, (0, 0, 0)]
    h0 = t.height
    assert h0 == 1 << 18, h0
    cols = np.concatenate([np.ascontiguousarray(t.base_array())] + list(t.ext_columns), axis=0)      # 7 + 12 planes of h0 words
    src = DeviceBuffer.from_numpy(cols.reshape(-1))
    ch = (u64 * 33)(*[v for c in challenges for v in c])
    tm = (u64 * 15)(*[v for c in terminals for v in c])
    results = []
    for log in [int(v) for v in args.logs.split(",")]:
        rows = 1 << log
        buf = DeviceBuffer(19 * rows)
        for c in range(19):
            for k in range(rows // h0):
                _lib.check(lib.bfs_memcpy_d2d(buf.ptr + 8 * (c * rows + k * h0), src.ptr + 8 * c * h0, 8 * h0, stream))
        for extended in (0, 1):
            nq = 21 if extended else 11
            out = (_lib.AirViolation * nq)()

            def call():
                _lib.check(lib.bfs_air_check(0, extended, buf.ptr, buf.ptr + 8 * 7 * rows, rows, rows, ch, tm, None, out, stream))
            for _ in range(3):
                call()
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                call()
                times.append(time.perf_counter() - t0)
            med = sorted(times)[len(times) // 2]
            nbytes = (7 + (12 if extended else 0)) * 8 * rows
            failing = sum(o.count for o in out)
            rec = {"rows": "2^%d" % log, "mode": "full" if extended else "base", "median_us": round(med * 1e6, 1),
                   "min_us": round(min(times) * 1e6, 1), "GB_per_s": round(nbytes / med / 1e9, 1), "failing_rows": int(failing)}
            results.append(rec)
            print(json.dumps(rec), flush=True)
        buf.free()
    return results


if __name__ == "__main__":
    main()
