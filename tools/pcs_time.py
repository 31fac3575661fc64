"""Times the opening of committed polynomials at out-of-domain points (stark_brainfuck_amd/pcs.py, csrc/deep.hip) at N = 2^22,
expansion 4, 16 base + 4 extension polynomials of 2^20 coefficients, k = 2 points: HIP events around each call after one warm-up call
of the same shape, the median of --reps calls per line (ms):

    evaluation      bfs_poly_eval_points over the 28 coefficient columns (one call, batch 28), and as `open` makes it (separate arrays, one read-back)
    quotient        bfs_deep_quotient over the 20 codewords; bfsx_deep_quotient_groups over the same codewords as one group at the same
                    points, and as a STARK's plan (7 groups, 6 distinct points, 11 pairs)
    open            PolynomialCommitment.open as a whole (host clock, ends in the stream synchronise of Fri.prove's read-backs)
    combination     bfs_combination over the same 20 codewords as sources (what the quotient is compared with)
    extension       bfs_gl_ntt of the same 28 columns from 2^20 coefficients to the 2^22 coset (what the evaluation is compared with)
    rounds          openings across commitments (rounds_leg): the STARK plan through bfsr_deep_quotient_rounds beside repeated measurements of
                    bfsx_deep_quotient_groups; a 64-column plan over three commitments (two launches) against bfsx_deep_quotient_groups on
                    its two halves; one open_rounds of the three commitments against three open_at (host clock, proof bytes)

and the shader clock sampled under a loop of quotient launches.  The numbers of profiles/pcs.md come from one run of this.

    python tools/pcs_time.py [--reps 7] [--log-n 22]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import stark_brainfuck_amd as sb
from stark_brainfuck_amd import _lib, pcs
from stark_brainfuck_amd.arrays import raw_ntt
from stark_brainfuck_amd.device import DeviceBuffer, current_stream, synchronize

EXPANSION, N_BASE, N_EXT, K, T = 4, 16, 4, 2, 8
u64 = ctypes.c_uint64


def timed(fn, reps):
    fn()                                                      # warm-up: tables, pool blocks
    synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--log-n", type=int, default=22)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lib = _lib.load()
    N = 1 << args.log_n
    d = N // EXPANSION
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    P = BF.p
    fri = sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, EXPANSION, T, XF)
    pc = sb.PolynomialCommitment(fri)
    rng = np.random.default_rng(1)
    columns = 3 * N_EXT + N_BASE
    coeffs = DeviceBuffer.from_numpy(rng.integers(0, P, size=columns * d, dtype=np.uint64))
    polys = [sb.XArray(_view(coeffs, 3 * e * d, 3 * d), d, XF) for e in range(N_EXT)]
    polys += [sb.BaseArray(_view(coeffs, (3 * N_EXT + b) * d, d), d) for b in range(N_BASE)]
    points = [XF.from_limbs([int(v) for v in rng.integers(1, P, size=3, dtype=np.uint64)]) for _ in range(K)]
    pts = [tuple(z.limbs()) for z in points]
    flat = (u64 * (3 * K))(*[v for z in pts for v in z])
    out = DeviceBuffer(3 * columns * K)
    stream = current_stream()
    report = {"log_n": args.log_n, "coefficients": d, "base_polynomials": N_BASE, "extension_polynomials": N_EXT, "points": K, "reps": args.reps}

    report["evaluation_one_call_ms"] = timed(lambda: _lib.check(lib.bfs_poly_eval_points(coeffs.ptr, d, d, columns, flat, K, out.ptr, stream)), args.reps)
    uncommitted = pcs.Commitment(polys, [isinstance(f, sb.XArray) for f in polys], list(range(len(polys))), None, N, None)      # (row order is the list's)
    all_columns = pc._one_group(pts, len(polys))                 # (`open` builds its plan once, in front of the evaluation)
    report["evaluation_as_open_ms"] = timed(lambda: pc._plan_values(all_columns, [uncommitted]), args.reps)
    codewords = DeviceBuffer(columns * N)
    report["extension_ms"] = timed(lambda: raw_ntt(coeffs.ptr, d, d, codewords.ptr, N, args.log_n, columns, pc.omega, pc.offset, 1, stream), args.reps)

    ps = sb.ProofStream()
    t0 = time.perf_counter()
    committed = pc.commit(polys, ps)
    synchronize()
    report["commit_wall_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
    values = [[(1 + j, 2 + p, 3) for p in range(N_BASE + N_EXT)] for j in range(K)]      # (the kernel's time does not depend on the claims)
    lam = (5, 6, 7)
    report["quotient_ms"] = timed(lambda: pc.quotient(committed, pts, values, lam), args.reps)

    # the same codewords through bfsx_deep_quotient_groups: as ONE group at the same two points, and in the shape a STARK asks for --
    # 7 groups, 6 distinct points (z, and z times one factor per table), 11 (group, point) pairs
    m = N_BASE + N_EXT
    one = pc.plan([(list(range(m)), pts)], m)
    report["quotient_one_group_ms"] = timed(lambda: pc.quotient_at(committed, one, [values], lam), args.reps)
    z = pts[0]
    nexts = [tuple(v * pow(pc.omega, 1 << (3 + i), P) % P for v in z) for i in range(5)]
    sizes, where = [4, 3, 3, 3, 2, 3, 2], [[z, nexts[0]], [z, nexts[1]], [z, nexts[2]], [z, nexts[3]], [nexts[4]], [z], [z]]
    firsts = [sum(sizes[:g]) for g in range(len(sizes))]
    stark = pc.plan([(list(range(first, first + size)), points_g) for first, size, points_g in zip(firsts, sizes, where)], m)
    assert (len(stark.groups), len(stark.points), stark.pairs) == (7, 6, 11)
    stark_values = [[[(1 + j, 2 + r, 3) for r in range(len(columns))] for j in range(len(indices))] for columns, indices in stark.groups]
    report["quotient_stark_plan_ms"] = timed(lambda: pc.quotient_at(committed, stark, stark_values, lam), args.reps)
    report["quotient_again_ms"] = timed(lambda: pc.quotient(committed, pts, values, lam), args.reps)      # (the old kernel once more: its run-to-run spread)

    sources = (_lib.CombSource * (N_BASE + N_EXT))()
    for c in range(N_BASE + N_EXT):
        s = sources[c]
        s.ptr, s.is_ext, s.pad, s.shift = committed.column_ptr(c), int(c < N_EXT), 0, 0
        for l in range(3):
            s.wa[l], s.wb[l] = 11 + c + l, 0
    randomizer = sb.XArray.empty(N, XF)
    lib.bfs_memset(randomizer.ptr, 0, 24 * N, stream)
    comb = sb.XArray.empty(N, XF)
    report["combination_ms"] = timed(lambda: _lib.check(lib.bfs_combination(sources, N_BASE + N_EXT, randomizer.ptr, (u64 * 3)(1, 0, 0), comb.ptr, args.log_n,
                                                                          pc.offset, pc.omega, stream)), args.reps)

    def whole_open():
        stream_ = sb.ProofStream()
        stream_.push(committed.root())
        pc.open(committed, points, stream_)
        synchronize()
    whole_open()
    wall = []
    for _ in range(args.reps):
        t = time.perf_counter()
        whole_open()
        wall.append(1e3 * (time.perf_counter() - t))
    report["open_wall_ms"] = (round(statistics.median(wall), 3), round(min(wall), 3), round(max(wall), 3))

    rounds_leg(report, pc, lib, args, committed, stark, stark_values, lam, rng, XF, P)

    # the shader clock half a second into a loop of quotient launches
    import bench
    stop = []

    def load():
        while not stop:
            for _ in range(20):
                pc.quotient(committed, pts, values, lam)
            synchronize()
    worker = threading.Thread(target=load)
    worker.start()
    report["clock_under_quotient_load"] = bench.sample_clock_under_load(0, delay_s=0.5)
    stop.append(1)
    worker.join()
    report["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(report), flush=True)


def _wall(fn, reps):
    fn()
    wall = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        wall.append(1e3 * (time.perf_counter() - t))
    return round(statistics.median(wall), 3), round(min(wall), 3), round(max(wall), 3)


def rounds_leg(report, pc, lib, args, first, stark, stark_values, lam, rng, XF, P):
    """openings across commitments (PolynomialCommitment.open_rounds, bfsr_deep_quotient_rounds):
    (a) the STARK plan above -- one launch -- through the new entry, beside two more measurements of bfsx_deep_quotient_groups (its spread);
    (b) 64 columns of three commitments in 8 groups of 8, two launches, against bfsx_deep_quotient_groups on the two halves;
    (c) one open_rounds of the three commitments against three open_at, in time and proof bytes"""
    N, d, reps = 1 << args.log_n, (1 << args.log_n) // EXPANSION, args.reps
    u32 = ctypes.c_uint32
    launches = u32(0)
    one = pc.rounds_plan(stark, [N_BASE + N_EXT])
    report["rounds_stark_plan_ms"] = timed(lambda: pc.quotient_rounds([first], one, stark_values, lam, launches), reps)
    assert launches.value == 1
    report["rounds_stark_plan_groups_entry_ms"] = [timed(lambda: pc.quotient_at(first, stark, stark_values, lam), reps) for _ in range(2)]
    report["rounds_stark_plan_again_ms"] = timed(lambda: pc.quotient_rounds([first], one, stark_values, lam, launches), reps)

    # two more commitments: 4 extension + 18 base polynomials, and 22 base polynomials: 20 + 22 + 22 = 64 columns
    shapes = [(4, 18), (0, 22)]
    commitments, ps = [first], sb.ProofStream()
    ps.push(first.root())
    for n_ext, n_base in shapes:
        coeffs = DeviceBuffer.from_numpy(rng.integers(0, P, size=(3 * n_ext + n_base) * d, dtype=np.uint64))
        polys = [sb.XArray(_view(coeffs, 3 * e * d, 3 * d), d, XF) for e in range(n_ext)]
        polys += [sb.BaseArray(_view(coeffs, (3 * n_ext + b) * d, d), d) for b in range(n_base)]
        commitments.append(pc.commit(polys, ps))
    widths = [len(c.polys) for c in commitments]
    assert sum(widths) == 64
    z = tuple(int(v) for v in rng.integers(1, P, size=3, dtype=np.uint64))
    nexts = [tuple(v * pow(pc.omega, 1 << (3 + i), P) % P for v in z) for i in range(4)]
    raw = [(list(range(8 * g, 8 * g + 8)), [z, nexts[g % 4]]) for g in range(8)]
    plan = pc.rounds_plan(raw, widths)
    values = [[[(1 + j, 2 + r, 3) for r in range(8)] for j in range(2)] for _ in range(8)]
    report["rounds_64_columns_ms"] = timed(lambda: pc.quotient_rounds(commitments, plan, values, lam, launches), reps)
    assert launches.value == 2
    where = [(c, k) for c in commitments for k in range(len(c.polys))]

    def half(first_group, g):
        """bfsx_deep_quotient_groups over four of the eight groups (32 columns, one launch)"""
        part = pc.plan([(list(range(8 * k, 8 * k + 8)), points) for k, (_, points) in enumerate(raw[first_group:first_group + 4])], 32)
        cols = (_lib.RowColumn * 32)()
        for at in range(32):
            c, k = where[8 * first_group + at]
            cols[at].d_values, cols[at].is_ext, cols[at].field_id = c.column_ptr(k), int(k < c.n_ext), 1
        combined, _ = part.combined_values(values[:4], lam)
        _lib.check(lib.bfsx_deep_quotient_groups(
            cols, 32, N, args.log_n, pc.offset, pc.omega, (u32 * 4)(*[8] * 4), (u32 * 4)(*[2] * 4), 4, pcs._flat_points(part.points), len(part.points),
            (u32 * part.pairs)(*[p for _, indices in part.groups for p in indices]), pcs._flat_points([y for per_group in combined for y in per_group]),
            (u64 * 3)(*lam), g.ptr, g.stride, current_stream()))
    g_half = sb.XArray.empty(N, XF)
    report["rounds_64_columns_halves_ms"] = [timed(lambda: half(0, g_half), reps), timed(lambda: half(4, g_half), reps)]

    # (c) one proof against three
    sizes = {}

    def one_proof():
        stream = sb.ProofStream()
        pc.open_rounds(commitments, plan, stream)
        synchronize()
        sizes["open_rounds"] = len(stream.serialize())

    def three_proofs():
        total = 0
        for c in commitments:
            m = len(c.polys)
            own = [(list(range(first_column, min(first_column + 8, m))), [z, nexts[g % 4]]) for g, first_column in enumerate(range(0, m, 8))]
            stream = sb.ProofStream()
            pc.open_at(c, own, stream)
            synchronize()
            total += len(stream.serialize())
        sizes["open_at_three"] = total
    report["open_rounds_wall_ms"] = _wall(one_proof, reps)
    report["open_at_three_wall_ms"] = _wall(three_proofs, reps)
    report["open_rounds_again_wall_ms"] = _wall(one_proof, reps)
    report["proof_bytes"] = sizes


def _view(buf, offset, count):
    from stark_brainfuck_amd.device import DeviceView
    return DeviceView(buf, offset, count)


if __name__ == "__main__":
    main()
