"""Times proof-of-work grinding in FRI: the nonce search on its own, Fri.prove at equal conjectured security with and without
grinding, and grinding_bits=0 against another build of the library (A/B).

    python tools/fri_grinding_time.py [--sizes 20,24] [--reps 20] [--other-lib PATH] [--json FILE]

One process, every shape warmed before it is timed, a host clock around calls that end in a stream synchronise, the variants
alternated call by call -- the method of tools/fri_folding_time.py, whose codeword, statistics and A/B series this tool uses.

  1. bfs_pow_search at 16, 24 and 32 bits over fixed seeds: median time to the nonce, and the rate in hashes per second over the
     launches the search made (it stops at the first launch with a hit: a launch is 2^(bits + 2) nonces, 2^24 at the most).  At 40
     bits one window of 2^35 nonces, a second or two of full launches: the kernel's sustained rate, with the shader clock sampled.
  2. Fri.prove (the Python call, fresh ProofStream each time), N = 2^size, expansion 4, for pairs (t, b) of colinearity tests and
     grinding bits with the same t * log2(expansion) + b: (8, 0) / (4, 8) / (2, 12) and (16, 0) / (8, 16), folding by 2 per element
     ("2") and by 8 with coset leaves ("8c"): median and fastest time, serialized proof bytes.
  3. with --other-lib: bfs_fri_prove and bfs_xfe_fold (grinding off: the default path) of THIS build and of the library at PATH (e.g.
     one built from the parent commit), as two interleaved series each; the distance between the medians of one build's two series
     is the spread of the run.
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import fri_folding_time as base  # noqa: E402

EXPANSION, OFFSET = base.EXPANSION, base.OFFSET
PAIRS = [[(8, 0), (4, 8), (2, 12)], [(16, 0), (8, 16)]]
MODES = {"2": (2, False), "8c": (8, True)}
LAUNCH_MAX_LOG2 = 24


def search_rates(lib, _lib, seeds=8):
    out = {}
    u64 = ctypes.c_uint64

    def search(seed, bits, count):
        nonce, found = u64(), ctypes.c_int()
        t0 = time.perf_counter()
        _lib.check(lib.bfs_pow_search(seed, bits, 0, count, ctypes.byref(nonce), ctypes.byref(found), 0))
        return time.perf_counter() - t0, (nonce.value if found.value else None)

    search(hashlib.sha256(b"warm").digest(), 16, 1 << 22)
    for bits in (16, 24, 32):
        step = 1 << min(bits + 2, LAUNCH_MAX_LOG2)
        times, hashes = [], []
        for i in range(seeds):
            dt, nonce = search(hashlib.sha256(b"rate %d %d" % (bits, i)).digest(), bits, 1 << (bits + 6))
            assert nonce is not None
            times.append(dt * 1e3)
            hashes.append((nonce // step + 1) * step)
        out[str(bits)] = {"median_ms_to_nonce": round(statistics.median(times), 4), "min_ms": round(min(times), 4),
                          "hashes_per_s": round(sum(hashes) / (sum(times) * 1e-3)), "launch_nonces": step}
    # the sustained rate: 2^35 nonces at 40 bits, 2 048 full launches unless one of them holds a hit (3 in 100), with the shader clock
    # sampled half a second into it (bench.sample_clock_under_load: what the integer-issue bound has to be priced at)
    import threading
    import bench
    got = {}
    worker = threading.Thread(target=lambda: got.update(zip(("s", "nonce"), search(hashlib.sha256(b"sustained").digest(), 40, 1 << 35))))
    worker.start()
    clock = bench.sample_clock_under_load(0, delay_s=0.5)
    worker.join()
    scanned = (1 << 35) if got["nonce"] is None else (got["nonce"] // (1 << 24) + 1) << 24
    out["sustained"] = {"hashes": scanned, "seconds": round(got["s"], 4), "hashes_per_s": round(scanned / got["s"]),
                        "sclk_mhz_sampled": (clock or {}).get("sclk_mhz_under_load")}
    return out


def prove_pairs(lib, _lib, log_n, reps):
    import stark_brainfuck_amd as sb
    N = 1 << log_n
    d_cw, _ = base._codeword(lib, _lib, log_n)
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    cw = sb.XArray(d_cw, N, XF, N)
    variants = [(mode, t, b) for mode in MODES for group in PAIRS for t, b in group]
    fris = {(mode, t, b): sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, EXPANSION, t, XF, folding_factor=MODES[mode][0],
                                 coset_leaves=MODES[mode][1], grinding_bits=b) for mode, t, b in variants}
    out = {v: {"ms": []} for v in variants}

    def call(v):
        ps = sb.ProofStream()
        t0 = time.perf_counter()
        fris[v].prove(cw, ps)
        _lib.check(lib.bfs_stream_synchronize(0))
        return (time.perf_counter() - t0) * 1e3, ps

    for v in list(variants):
        try:
            for _ in range(2):
                _, ps = call(v)
        except AssertionError as refused:       # more tests than the last codeword has elements (folding by 2 ends at 2 * expansion)
            out[v] = {"refused": str(refused)}
            variants.remove(v)
            continue
        out[v]["proof_bytes"], out[v]["objects"] = len(ps.serialize()), len(ps.objects)
    for _ in range(reps):
        for v in variants:
            out[v]["ms"].append(call(v)[0])
    d_cw.free()
    return {"%s t=%d b=%d" % v: (dict(base._stats(r.pop("ms")), **r) if "ms" in r else r) for v, r in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    from stark_brainfuck_amd import _lib
    lib = _lib.load()
    other = base._bind(os.path.abspath(args.other_lib), _lib) if args.other_lib else None
    result = {"expansion": EXPANSION, "reps": args.reps, "search": search_rates(lib, _lib), "sizes": {}}
    print("nonce search (bfs_pow_search from nonce 0)")
    for bits in ("16", "24", "32"):
        r = result["search"][bits]
        print("  %2s bits  median %9.3f ms to the nonce (fastest %.3f)  %.3e hashes/s over launches of 2^%d nonces" % (
            bits, r["median_ms_to_nonce"], r["min_ms"], r["hashes_per_s"], r["launch_nonces"].bit_length() - 1))
    r = result["search"]["sustained"]
    print("  sustained, %d nonces at 40 bits in %.3f s: %.3e hashes/s, shader clock sampled under it: %s MHz" % (
        r["hashes"], r["seconds"], r["hashes_per_s"], r["sclk_mhz_sampled"]))
    sys.stdout.flush()
    for log_n in [int(x) for x in args.sizes.split(",")]:
        entry = {"prove": prove_pairs(lib, _lib, log_n, args.reps)}
        print("N = 2^%d  Fri.prove, expansion %d  (security = t * log2(expansion) + b; 8c = folding by 8 with coset leaves)" % (log_n, EXPANSION))
        print("  mode  tests  bits  objects  proof bytes   median / min ms")
        for name, r in entry["prove"].items():
            mode, t, b = name.split()
            if "refused" in r:
                print("  %4s  %5s  %4s  refused: %s" % (mode, t[2:], b[2:], r["refused"]))
                continue
            print("  %4s  %5s  %4s  %7d  %11d   %9.3f / %-9.3f" % (mode, t[2:], b[2:], r["objects"], r["proof_bytes"], r["median_ms"], r["min_ms"]))
        if other is not None:
            entry["ab"] = base.ab_folding_two(lib, other, _lib, log_n, args.reps)
            for what, r in entry["ab"].items():
                print("  A/B %-14s this %.4f ms  other %.4f ms  difference %+.4f ms  spread of this run %.4f ms  -> %s" % (
                    what, r["this_ms"], r["other_ms"], r["difference_ms"], r["spread_ms"], "within the spread" if r["within_spread"] else "BEYOND the spread"))
        sys.stdout.flush()
        result["sizes"][str(log_n)] = entry
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
