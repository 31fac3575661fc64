#!/usr/bin/env python3
"""Byte-level mutation fuzzing of the native proof reader and verifier (round-5 verdict, next #3).

verify() gives attacker-controlled bytes to csrc/refpickle.hpp (bfs_ps_loads) and walks the resulting object graph in
csrc/verifier.cpp; the reference does the same with CPython's pickle.loads (/root/reference/code/ip.py:27-30) and its Python verifier
(brainfuck_stark.py:343-579, fri.py:201-319).  This tool mutates the bytes of every golden proof under tests/golden/ and pushes each
mutant through (1) the native reader, (2) the native verifier when the reader took it, (3) the Python verifier where the native route
declines.  A run passes when nothing crashes, no sanitizer reports (run it on the hardening build:

    python -m stark_brainfuck_amd.build --sanitize          # prints the library and the runtime to preload
    LD_PRELOAD=<runtime> ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 BFS_LIB_PATH=stark_brainfuck_amd/libbfstark_hip_asan.so \\
        python tools/fuzz_proofs.py --mutants 5000

) and no mutant is ACCEPTED unless its object stream is the original's (a re-encoding of the same proof is the same proof).
tests/test_sanitized_parsers.py runs it that way inside the CPU suite; no GPU is needed."""
import argparse
import glob
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

INTERESTING = [0x00, 0x01, 0x7F, 0x80, 0xFF, 0x2E, 0x28, 0x29, 0x5D, 0x61, 0x65, 0x85, 0x86, 0x87, 0x8A, 0x8B, 0x42, 0x43, 0x8E, 0x94, 0x95,
               0x68, 0x6A, 0x71, 0x72, 0x4A, 0x4B, 0x4D, 0x51, 0x52, 0x62, 0x81, 0x93, 0x8C, 0x58, 0x30, 0x31, 0x32, 0x4E, 0x74, 0x75]
SAVE_LAST = os.environ.get("BFS_FUZZ_SAVE_LAST")
WORDS = [0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xFFFFFFFE, 64, 65, 255, 256, 1 << 20, 1 << 24, 1 << 30]


def mutate(rnd, data, others):
    b = bytearray(data)
    for _ in range(rnd.choice((1, 1, 1, 2, 3, 8))):
        how = rnd.randrange(12)
        n = len(b)
        if n == 0:
            break
        k = rnd.randrange(n)
        if how == 0:
            b[k] ^= 1 << rnd.randrange(8)
        elif how == 1:
            b[k] = rnd.choice(INTERESTING)
        elif how == 2:
            b[k] = rnd.randrange(256)
        elif how == 3:                                       # delete a range
            del b[k:k + rnd.choice((1, 2, 4, 8, 64, 1024))]
        elif how == 4:                                       # duplicate a range
            m = rnd.choice((1, 2, 8, 64, 409, 4096))
            b[k:k] = b[k:k + m]
        elif how == 5:                                       # insert noise / opcodes
            b[k:k] = bytes(rnd.choice(INTERESTING) if rnd.random() < 0.7 else rnd.randrange(256) for _ in range(rnd.choice((1, 2, 4, 16))))
        elif how == 6:                                       # truncate
            del b[rnd.randrange(n):]
        elif how == 7 and n >= 4:                            # a 4-byte little-endian field (frame / bytes / memo lengths)
            k = rnd.randrange(n - 3)
            b[k:k + 4] = rnd.choice(WORDS).to_bytes(4, "little")
        elif how == 8 and n >= 8:                            # an 8-byte field (FRAME, BINBYTES8)
            k = rnd.randrange(n - 7)
            b[k:k + 8] = rnd.choice(WORDS + [1 << 40, (1 << 63) - 1, (1 << 64) - 1]).to_bytes(8, "little")
        elif how == 9 and others:                            # splice a range of another proof in
            o = rnd.choice(others)
            j = rnd.randrange(len(o))
            m = rnd.choice((8, 64, 512, 4096))
            b[k:k + m] = o[j:j + m]
        elif how == 10:                                      # swap two ranges
            m = rnd.choice((1, 8, 64))
            j = rnd.randrange(n)
            b[k:k + m], b[j:j + m] = b[j:j + m], b[k:k + m]
        else:                                                # set a run
            m = rnd.choice((2, 8, 32))
            b[k:k + m] = bytes([rnd.choice((0, 0xFF, 0x80))]) * min(m, n - k)
    return bytes(b)


def stark_of(name):
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    from stark_brainfuck_amd.vm import VirtualMachine
    g = json.load(open(os.path.join(GOLDEN, "stark_%s.json" % name)))
    program = VirtualMachine.compile(g["program"])
    running_time, input_symbols, output_symbols = VirtualMachine.run(program, input_data=list(g["input"]))
    _, mm, _, _, _ = VirtualMachine.simulate(program, input_data=list(input_symbols))
    return BrainfuckStark(running_time, len(mm), program, input_symbols, output_symbols)


def same_objects(a, b):
    from stark_brainfuck_amd import ProofStream
    try:
        return repr(ProofStream().deserialize(a).objects) == repr(ProofStream().deserialize(b).objects)
    except Exception:  # noqa: BLE001
        return False


def fuzz_one(name, mutants, seed, python_sample, others):
    from stark_brainfuck_amd.ip import NativeTranscript
    proof = open(os.path.join(GOLDEN, "stark_%s_proof.bin" % name), "rb").read()
    stark = stark_of(name)
    assert stark.verify(proof) is True, name
    rnd = random.Random(seed)
    stats = {"name": name, "bytes": len(proof), "mutants": 0, "refused_by_reader": 0, "native_false": 0, "native_assert": 0, "native_declined": 0,
             "native_true_same_objects": 0, "steered_into_verifier": 0, "python_route": 0, "python_false_or_raise": 0, "accepted": []}
    good = []                      # byte positions at which a point mutation got past the reader (payload bytes): reused by the steering below
    i = -1
    while stats["mutants"] < mutants:
        i += 1
        mut = mutate(rnd, proof, others)
        if mut == proof:
            continue
        stats["mutants"] += 1
        if SAVE_LAST:
            with open(SAVE_LAST, "wb") as f:          # a crash leaves the input that caused it behind
                f.write(mut)
        t = NativeTranscript.from_bytes(mut)
        if t is None and i % 2 == 1:
            # every other mutant is made to REACH the verifier: four out of five random mutants die in the reader's framing checks, so
            # point mutations (a bit, a byte) are retried until the reader takes the stream -- payload bytes of integers, digests and salts
            for _ in range(12):
                b = bytearray(proof)
                ks = []
                for _ in range(rnd.choice((1, 1, 2, 4))):
                    k = rnd.choice(good) if len(good) >= 64 and rnd.random() < 0.8 else rnd.randrange(len(b))
                    ks.append(k)
                    b[k] = b[k] ^ (1 << rnd.randrange(8)) if rnd.random() < 0.6 else rnd.randrange(256)
                mut = bytes(b)
                if SAVE_LAST:
                    with open(SAVE_LAST, "wb") as f:
                        f.write(mut)
                t = NativeTranscript.from_bytes(mut) if mut != proof else None
                if t is not None:
                    stats["steered_into_verifier"] += 1
                    if len(good) < 4096:
                        good.extend(ks)
                    break
        if t is None:
            stats["refused_by_reader"] += 1
            route_python = rnd.random() < python_sample
        else:
            del t
            try:
                verdict = stark._verify_native(mut)
            except AssertionError:
                stats["native_assert"] += 1
                continue
            if verdict is False:
                stats["native_false"] += 1
                continue
            if verdict is True:
                if same_objects(mut, proof):
                    stats["native_true_same_objects"] += 1
                else:
                    stats["accepted"].append({"mutant": i, "route": "native", "hex_diff_at": next(k for k in range(min(len(mut), len(proof))) if mut[k] != proof[k])})
                continue
            stats["native_declined"] += 1
            route_python = True
        if route_python:
            stats["python_route"] += 1
            try:
                v = stark.verify(mut)
            except Exception:  # noqa: BLE001 -- the reference's verifier raises on malformed streams too (pickle errors, assertions)
                v = False
            if v is True and not same_objects(mut, proof):
                stats["accepted"].append({"mutant": i, "route": "python"})
            else:
                stats["python_false_or_raise"] += 1
    return stats


def write_params(name, path):
    """the claim's protocol parameters and degree shifts as a flat file of little-endian words, for tools/fuzz_ps_loads.cpp"""
    import struct
    stark = stark_of(name)
    proof = open(os.path.join(GOLDEN, "stark_%s_proof.bin" % name), "rb").read()
    n = stark.fri.domain.length
    distances = stark._layout.unit_distances(n)
    words = [n.bit_length() - 1, stark.expansion_factor, stark.num_colinearity_checks, stark.security_level, stark.fri.domain.offset.value, stark.fri.domain.omega.value]
    words += [t.height for t in stark.tables] + [t.length for t in stark.tables] + [t.omicron.value for t in stark.tables]
    words += [len(distances)] + distances + [0] * (8 - len(distances))
    program = [w.value if hasattr(w, "value") else int(w) for w in stark.program]
    # the degree shifts depend on challenges and terminals of the proof at hand (brainfuck_stark.py:203-221): take the golden proof's
    assert stark.verify(proof) is True
    g = json.load(open(os.path.join(GOLDEN, "stark_%s.json" % name)))
    challenges = tuple(tuple(c) for c in g["quotients"][0]["challenges"])
    terminals = [tuple(t) for t in g["terminals"]]
    shifts = stark._layout.shifts(stark._quotient_degree_bounds(challenges, terminals, cached=True))
    for seq in (program, [ord(c) for c in stark.input_symbols], [ord(c) for c in stark.output_symbols], shifts):
        words += [len(seq)] + list(seq)
    with open(path, "wb") as f:
        f.write(struct.pack("<%dQ" % len(words), *words))
    print(json.dumps({"name": name, "params": path, "words": len(words), "proof_bytes": len(proof), "BFS_FUZZ_ACCEPT_SIZE": len(proof)}))


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--write-params":
        return write_params(sys.argv[2], sys.argv[3])
    ap = argparse.ArgumentParser()
    ap.add_argument("--mutants", type=int, default=5000, help="per golden proof")
    ap.add_argument("--seed", type=int, default=20261001)
    ap.add_argument("--names", default="", help="comma-separated fixture names (default: every stark_*_proof.bin)")
    ap.add_argument("--python-sample", type=float, default=0.02, help="share of reader-refused mutants also given to the Python verifier")
    ap.add_argument("--max-bytes", type=int, default=1 << 20)
    args = ap.parse_args()
    names = [n for n in args.names.split(",") if n] or sorted(os.path.basename(f)[6:-10] for f in glob.glob(os.path.join(GOLDEN, "stark_*_proof.bin")))
    blobs = {n: open(os.path.join(GOLDEN, "stark_%s_proof.bin" % n), "rb").read() for n in names}
    t0 = time.time()
    total = {"mutants": 0, "accepted": 0}
    for n in names:
        if len(blobs[n]) > args.max_bytes:
            continue
        s = fuzz_one(n, args.mutants, args.seed ^ hash(n) & 0xFFFF, args.python_sample, [b for m, b in blobs.items() if m != n])
        total["mutants"] += s["mutants"]
        total["accepted"] += len(s["accepted"])
        print(json.dumps(s), flush=True)
    total["seconds"] = round(time.time() - t0, 1)
    from stark_brainfuck_amd import _lib
    total["library"] = _lib.LIB_PATH
    print(json.dumps(total), flush=True)
    sys.exit(1 if total["accepted"] else 0)


if __name__ == "__main__":
    main()
