"""Times the GPU subproduct tree (SubproductTree: bfs_ptree_build / _evaluate / _interpolate) at 2^12 .. 2^20 random base-field
points, for 1 and 8 base columns, with HIP events around each call after one warm-up call of the same shape; the median of --reps
calls is printed per line (ms).  Also the list-API fast_interpolate of a 4 096-row table column as Table.interpolate_columns makes
it (lifted omicron domain + 4 randomizer points, extension values), wall clock including the object conversions.

    python tools/ptree_time.py [--reps 5] [--logs 12,14,16,18,20]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import stark_brainfuck_amd as sb


def timed(fn, reps):
    fn()                                                      # warm-up: tables, pool blocks
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--logs", default="12,14,16,18,20")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    P = sb.BaseField.main().p
    rng = np.random.default_rng(1)
    for log_n in (int(x) for x in args.logs.split(",")):
        n = 1 << log_n
        pts = sb.BaseArray.from_numpy(rng.integers(0, P, size=n, dtype=np.uint64))
        build = timed(lambda: sb.SubproductTree(pts).free(), args.reps)
        tree = sb.SubproductTree(pts)
        row = {"log_n": log_n, "build_ms": round(build, 3)}
        for cols in (1, 8):
            data = sb.BaseArray.from_numpy(rng.integers(0, P, size=(cols, n), dtype=np.uint64) if cols > 1 else
                                           rng.integers(0, P, size=n, dtype=np.uint64))
            row["evaluate_%d_ms" % cols] = round(timed(lambda: tree.evaluate(data), args.reps), 3)
            row["interpolate_%d_ms" % cols] = round(timed(lambda: tree.interpolate(data), args.reps), 3)
        tree.free()
        print(row, flush=True)
    XF = sb.ExtensionField.main()
    F = XF._base()
    order = 1 << 15
    omicron = F.primitive_nth_root(4096)
    domain = [XF.lift(omicron ^ i) for i in range(4096)] + [XF.lift(F.primitive_nth_root(order) ^ (2 * i + 1)) for i in range(4)]
    values = [XF.from_limbs([int(v) for v in rng.integers(0, P, size=3, dtype=np.uint64)]) for _ in range(len(domain))]
    root = XF.lift(F.primitive_nth_root(order))
    sb.fast_interpolate(domain, values, root, order)
    wall = []
    for _ in range(args.reps):
        t = time.perf_counter()
        sb.fast_interpolate(domain, values, root, order)
        wall.append((time.perf_counter() - t) * 1e3)
    print({"list_fast_interpolate_4100_lifted_xvalues_ms": round(statistics.median(wall), 3)}, flush=True)


if __name__ == "__main__":
    main()
