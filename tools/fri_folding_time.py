"""Times FRI with folding factors 2, 4 and 8, with one Merkle leaf per element and per folding coset (coset_leaves), and folding by 2
against another build of the library (A/B).

    python tools/fri_folding_time.py [--sizes 20,24] [--reps 30] [--other-lib PATH] [--stark] [--json FILE]

One process, every shape warmed before it is timed, a host clock around calls that end in a stream synchronise, the variants
alternated call by call (so drift of the clock or of the host hits all of them alike).  N = 2^size, expansion 4, 4 colinearity tests.

  1. Fri.prove (the Python call, fresh ProofStream each time) and bfs_fri_prove_cosets (the C ABI, codeword resident in HBM) for
     folding 2, 4, 8, each with per-element and with coset leaves: median and fastest time, proof bytes, number of stream objects, and
     the ratio coset / per-element at the same folding factor.
  2. with --other-lib: bfs_fri_prove and bfs_xfe_fold of THIS build and of the library at PATH (e.g. one built from the parent
     commit), both loaded into this process and alternated.  Each build is measured as two interleaved series; the distance between
     the medians of the two series of one build is the spread of this run, and the builds differ measurably only beyond it.
  3. with --stark and --other-lib: BrainfuckStark.prove on Hello World (bench.bench_stark), one child process per run because the
     package binds one library per process (BFS_LIB_PATH): this, other, this, other.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXPANSION, TESTS, OFFSET = 4, 4, 7
NEW_SYMBOLS = ("bfs_xfe_fold_multi", "bfs_fri_session_set_folding", "bfs_fri_prove_folded", "bfs_merkle_build_xfe_cosets", "bfs_coset_trees_by_rows",
               "bfs_fri_session_set_coset_leaves", "bfs_fri_session_round0_coset_tree", "bfs_fri_prove_cosets", "bfs_fri_session_round_leaves")


def _load_package_library():
    """stark_brainfuck_amd._lib.load(), tolerating a BFS_LIB_PATH build that predates the folding entry points"""
    from stark_brainfuck_amd import _lib
    probe = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        if not hasattr(probe, name):
            _lib._SIGNATURES.pop(name, None)
    return _lib, _lib.load()


def _bind(path, _lib):
    """another build of the library in this process: the signatures of the entry points this tool calls"""
    lib = ctypes.CDLL(path)
    for name in ("bfs_ps_new", "bfs_ps_free", "bfs_ps_serialize", "bfs_fri_prove", "bfs_xfe_fold", "bfs_stream_synchronize",
                 "bfs_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._SIGNATURES[name]
    return lib


def _stats(samples_ms):
    return {"median_ms": round(statistics.median(samples_ms), 4), "min_ms": round(min(samples_ms), 4), "n": len(samples_ms)}


def _codeword(lib, _lib, log_n):
    """a degree-(N/4 - 1) extension polynomial's evaluations over the coset, in HBM (as bench.bench_fri makes it)"""
    import bench
    from stark_brainfuck_amd.device import DeviceBuffer
    N = 1 << log_n
    d = N // EXPANSION
    omega = lib.bfs_gl_primitive_root(log_n)
    coeffs = bench.felt_array(bench.SEED, 0, 3 * d).reshape(d, 3).T.copy()
    d_coef = DeviceBuffer.from_numpy(coeffs.reshape(-1))
    d_cw = DeviceBuffer(3 * N)
    _lib.check(lib.bfs_gl_ntt(d_coef.ptr, d, d, d_cw.ptr, N, log_n, 3, omega, OFFSET, 1, 0))
    _lib.check(lib.bfs_stream_synchronize(0))
    return d_cw, omega


def _serialized_size(lib, ps):
    size = ctypes.c_size_t()
    lib.bfs_ps_serialize(ps, 1 << 62, None, 0, ctypes.byref(size))
    return size.value


def folding_variants(lib, _lib, log_n, reps):
    import stark_brainfuck_amd as sb
    N = 1 << log_n
    d_cw, omega = _codeword(lib, _lib, log_n)
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    cw = sb.XArray(d_cw, N, XF, N)
    # variant = (folding factor, coset leaves)
    fris = {(a, coset): sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, EXPANSION, TESTS, XF, folding_factor=a, coset_leaves=coset)
            for a in (2, 4, 8) for coset in (False, True)}
    out = {a: {"python_ms": [], "c_abi_ms": []} for a in fris}

    def python_call(a):
        ps = sb.ProofStream()
        t0 = time.perf_counter()
        fris[a].prove(cw, ps)
        _lib.check(lib.bfs_stream_synchronize(0))
        dt = time.perf_counter() - t0
        return dt, ps

    def c_call(a):
        ps = lib.bfs_ps_new()
        idx = (ctypes.c_uint64 * TESTS)()
        t0 = time.perf_counter()
        _lib.check(lib.bfs_fri_prove_cosets(ps, d_cw.ptr, N, log_n, OFFSET, omega, EXPANSION, a[0].bit_length() - 1, int(a[1]), TESTS, idx, 0))
        _lib.check(lib.bfs_stream_synchronize(0))
        dt = time.perf_counter() - t0
        return dt, ps

    for a in fris:                       # warm every shape; keep the size of the proof
        for _ in range(3):
            _, ps = python_call(a)
        out[a]["proof_bytes"], out[a]["objects"], out[a]["codewords"] = len(ps.serialize()), len(ps.objects), fris[a].num_rounds()
        for _ in range(3):
            _, ps = c_call(a)
            assert _serialized_size(lib, ps) == out[a]["proof_bytes"]
            lib.bfs_ps_free(ps)
    for _ in range(reps):
        for a in fris:
            out[a]["python_ms"].append(python_call(a)[0] * 1e3)
        for a in fris:
            dt, ps = c_call(a)
            lib.bfs_ps_free(ps)
            out[a]["c_abi_ms"].append(dt * 1e3)
    for a in fris:
        out[a]["python"], out[a]["c_abi"] = _stats(out[a].pop("python_ms")), _stats(out[a].pop("c_abi_ms"))
    d_cw.free()
    return {"%d%s" % (a, "c" if coset else ""): r for (a, coset), r in out.items()}


def _ab_report(series):
    """series: {'this': [[..], [..]], 'other': [[..], [..]]} in ms"""
    med = {k: [statistics.median(s) for s in v] for k, v in series.items()}
    both = {k: statistics.median(v[0] + v[1]) for k, v in series.items()}
    spread = max(abs(m[0] - m[1]) for m in med.values())
    diff = both["this"] - both["other"]
    return {"this_ms": round(both["this"], 4), "other_ms": round(both["other"], 4), "this_series_ms": [round(x, 4) for x in med["this"]],
            "other_series_ms": [round(x, 4) for x in med["other"]], "difference_ms": round(diff, 4), "spread_ms": round(spread, 4),
            "within_spread": abs(diff) <= spread}


def ab_folding_two(lib, other, _lib, log_n, reps):
    N = 1 << log_n
    d_cw, omega = _codeword(lib, _lib, log_n)
    from stark_brainfuck_amd.device import DeviceBuffer
    d_half = DeviceBuffer(3 * (N // 2))
    alpha = (ctypes.c_uint64 * 3)(5, 6, 7)
    builds = {"this": lib, "other": other}

    def prove(l):
        ps = l.bfs_ps_new()
        idx = (ctypes.c_uint64 * TESTS)()
        t0 = time.perf_counter()
        rc = l.bfs_fri_prove(ps, d_cw.ptr, N, log_n, OFFSET, omega, EXPANSION, TESTS, idx, 0)
        l.bfs_stream_synchronize(0)
        dt = time.perf_counter() - t0
        assert rc == 0, l.bfs_last_error()
        size = _serialized_size(l, ps)
        l.bfs_ps_free(ps)
        return dt * 1e3, (size, [int(x) for x in idx])

    def fold(l, calls=20):
        t0 = time.perf_counter()
        for _ in range(calls):
            rc = l.bfs_xfe_fold(d_cw.ptr, N, d_half.ptr, N // 2, log_n, alpha, OFFSET, omega, 0)
        l.bfs_stream_synchronize(0)
        assert rc == 0, l.bfs_last_error()
        return (time.perf_counter() - t0) * 1e3 / calls, None

    report = {}
    for what, call in (("bfs_fri_prove", prove), ("bfs_xfe_fold", fold)):
        same = set()
        for l in builds.values():
            for _ in range(3):
                same.add(repr(call(l)[1]))
        assert len(same) == 1, "the two builds disagree: %s" % same
        series = {k: [[], []] for k in builds}
        for rep in range(2 * reps):
            for k in (("this", "other") if rep % 4 < 2 else ("other", "this")):
                series[k][rep % 2].append(call(builds[k])[0])
        report[what] = _ab_report(series)
    d_cw.free(); d_half.free()
    return report


def _stark_child():
    _load_package_library()
    import bench
    r = bench.bench_stark()
    print("STARK_MS %.4f verified %s" % (r["ms"], r["verified"]))


def ab_stark(other_path):
    series = {"this": [], "other": []}
    for run in range(2):
        for k in ("this", "other"):
            env = dict(os.environ)
            env.pop("BFS_LIB_PATH", None)
            if k == "other":
                env["BFS_LIB_PATH"] = other_path
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--stark-child"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                 text=True, timeout=600)
            lines = [x for x in res.stdout.splitlines() if x.startswith("STARK_MS")]
            if res.returncode != 0 or not lines:
                raise RuntimeError("stark child failed:\n" + res.stdout[-2000:])
            assert lines[0].endswith("verified True"), lines[0]
            series[k].append([float(lines[0].split()[1])])
    return _ab_report(series)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--stark", action="store_true")
    ap.add_argument("--stark-child", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.stark_child:
        return _stark_child()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    _lib, lib = _load_package_library()
    other = _bind(os.path.abspath(args.other_lib), _lib) if args.other_lib else None
    result = {"expansion": EXPANSION, "colinearity_tests": TESTS, "reps": args.reps, "sizes": {}}
    for log_n in [int(x) for x in args.sizes.split(",")]:
        entry = {"folding": folding_variants(lib, _lib, log_n, args.reps)}
        print("N = 2^%d  (Fri.prove: Python call; C ABI: bfs_fri_prove_cosets; folding 4c = folding by 4 with coset leaves)" % log_n)
        print("  folding  codewords  objects  proof bytes   Fri.prove median / min ms    C ABI median / min ms   C ABI coset / per-element")
        for a, r in entry["folding"].items():
            ratio = "%.3f" % (r["c_abi"]["median_ms"] / entry["folding"][a[:-1]]["c_abi"]["median_ms"]) if a.endswith("c") else ""
            print("  %7s  %9d  %7d  %11d   %10.3f / %-10.3f   %10.3f / %-10.3f   %s" % (a, r["codewords"], r["objects"], r["proof_bytes"], r["python"]["median_ms"],
                                                                                     r["python"]["min_ms"], r["c_abi"]["median_ms"], r["c_abi"]["min_ms"], ratio))
        if other is not None:
            entry["ab"] = ab_folding_two(lib, other, _lib, log_n, args.reps)
            for what, r in entry["ab"].items():
                print("  A/B %-14s this %.4f ms  other %.4f ms  difference %+.4f ms  spread of this run %.4f ms  -> %s" % (
                    what, r["this_ms"], r["other_ms"], r["difference_ms"], r["spread_ms"], "within the spread" if r["within_spread"] else "BEYOND the spread"))
        sys.stdout.flush()
        result["sizes"][str(log_n)] = entry
    if args.stark and args.other_lib:
        result["stark_hello_world"] = r = ab_stark(os.path.abspath(args.other_lib))
        print("A/B BrainfuckStark.prove (Hello World)  this %s ms  other %s ms  difference %+.4f ms  spread %.4f ms  -> %s" % (
            r["this_series_ms"], r["other_series_ms"], r["difference_ms"], r["spread_ms"], "within the spread" if r["within_spread"] else "BEYOND the spread"))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
