"""BrainfuckStark in its FRI modes (folding_factor, coset_leaves, grinding_bits): proof size, prove and verify time per mode, and the
committed fixtures of the modes.

    python tools/stark_fri_modes.py [--program loop|plus1|hello|big|SOURCE] [--reps 7] [--json FILE]
    python tools/stark_fri_modes.py --write-golden DIR
    python tools/stark_fri_modes.py --ab PARENT_ROOT [--rounds 5]

Per mode of TABLE_MODES the tool proves the program `reps` times with fresh BrainfuckStark objects (the first proof of a shape warms it
and is dropped), verifies the last proof natively, and prints proof bytes, the median prove and verify time and the number of
authentication-path digests in the proof.  One process, a host clock around calls that end in a stream synchronise.

--ab PARENT_ROOT measures the default mode against a built checkout of the parent commit at PARENT_ROOT: alternating child processes
(parent, this, parent, this, ...), each proving and verifying "Hello World!" and the 2^11 program with the package of its tree; per
figure the medians over the processes and the parent's own max - min, which is the allowance.

--write-golden DIR writes the proofs of FIXTURES with the seeded randomness of tests/test_gpu_stark.py (os.urandom replaced by the
SHAKE-256 stream of the golden of the same program) and DIR/fri_modes_stark.json, which lists per file the program, the constructor
arguments and the proof's SHA-256.  The proofs need a GPU; everything the tests share with this tool -- the modes, the seeded stream,
the claims -- is importable without one.
"""
import argparse
import contextlib
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE_LIST = "fri_modes_stark.json"

# golden programs (tests/golden/stark_<name>.json): FRI domain 2^8 and 2^11 with the default expansion factor
PROGRAMS = {"plus1": "+", "loop": "++[>+<-]>."}
HELLO_WORLD = "++++++++[>++++[>++>+++>+++>+<<<<-]>+>+>->>+[<]<-]>>.>---.+++++++..+++.>>.<-.<.+++.------.--------.>>+.>++."
BIG = "+" * 64 + "[>" + "+" * 64 + "[>++++<-]<-]+++."          # nested loops, 37 254 cycles: FRI domain 2^22


def mode(folding_factor=2, coset_leaves=False, grinding_bits=0, log_expansion_factor=2, security_level=2):
    return {"log_expansion_factor": log_expansion_factor, "security_level": security_level, "folding_factor": folding_factor,
            "coset_leaves": coset_leaves, "grinding_bits": grinding_bits}


DEFAULT = mode()
# (program, mode) of every committed proof
# (grinding 4 needs security_level >= 6 for one colinearity check: (6 - 4) // 2)
FIXTURES = [("loop", mode(4)), ("loop", mode(8, True)), ("loop", mode(8, True, 4, security_level=6)), ("loop", mode(2, False, 4, security_level=6)),
            ("plus1", mode(8, True))]
TABLE_MODES = [mode(), mode(4), mode(8), mode(2, True), mode(4, True), mode(8, True), mode(8, True, 4, security_level=6), mode(2, False, 4, security_level=6),
               mode(security_level=6)]


def mode_id(m):
    tag = "a%d%s" % (m["folding_factor"], "c" if m["coset_leaves"] else "")
    if m["grinding_bits"]:
        tag += "_g%d" % m["grinding_bits"]
    if (m["log_expansion_factor"], m["security_level"]) != (2, 2):
        tag += "_e%d_s%d" % (m["log_expansion_factor"], m["security_level"])
    return tag


def fixture_file(name, m):
    return "fri_modes_%s_%s_proof.bin" % (name, mode_id(m))


class Stream:
    """the byte stream tests/golden/gen_stark_golden.py fed to the reference as os.urandom (tests/test_gpu_stark.py)"""

    def __init__(self, tag):
        self.tag, self.pos, self.buf = tag, 0, b""

    def __call__(self, n):
        end = self.pos + n
        if end > len(self.buf):
            self.buf = hashlib.shake_256(b"bfs-golden-urandom" + self.tag).digest(max(2 * end, 1 << 16))
        out = self.buf[self.pos:end]
        self.pos = end
        return out


@contextlib.contextmanager
def seeded(name):
    """every random draw of prove() from the stream of golden `name`"""
    from stark_brainfuck_amd import brainfuck_stark, salted_merkle, table
    stream = Stream(name.encode())
    saved = [(m, m.urandom) for m in (brainfuck_stark, salted_merkle, table)]
    try:
        for m, _ in saved:
            m.urandom = stream
        yield stream
    finally:
        for m, u in saved:
            m.urandom = u


_claims = {}


def claim(source):
    """(program, running_time, input symbols, output symbols, trace matrices) of a program without input"""
    from stark_brainfuck_amd.vm import VirtualMachine
    if source not in _claims:
        program = VirtualMachine.compile(source)
        running_time, inputs, outputs = VirtualMachine.run(program)
        _claims[source] = (program, running_time, inputs, outputs, VirtualMachine.simulate(program, input_data=inputs))
    return _claims[source]


def stark_args(source, m):
    """the positional arguments of BrainfuckStark for `source` in mode m"""
    program, running_time, inputs, outputs, matrices = claim(source)
    return (running_time, len(matrices[1]), program, inputs, outputs, m["log_expansion_factor"], m["security_level"], m["folding_factor"],
            m["coset_leaves"], m["grinding_bits"])


def make_stark(source, m):
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    return BrainfuckStark(*stark_args(source, m))


def prove_seeded(name, m, prepare=None, proof_stream=None):
    """-> (stark, proof) of golden program `name` in mode m on the golden's randomness; prepare(stark) runs before prove()"""
    source = PROGRAMS[name]
    stark = make_stark(source, m)
    if prepare is not None:
        prepare(stark)
    with seeded(name):
        proof = stark.prove(claim(source)[0], *claim(source)[4], proof_stream=proof_stream)
    return stark, proof


def fixtures(directory=GOLDEN):
    """the entries of fri_modes_stark.json: dicts with file, name, program, args, proof_len, proof_sha256"""
    path = os.path.join(directory, FIXTURE_LIST)
    if not os.path.exists(path):
        return []
    with open(path) as f:
        return json.load(f)["proofs"]


def count_digests(proof):
    """64-byte items of the lists among a proof's objects: authentication-path digests"""
    from stark_brainfuck_amd.ip import ProofStream

    def walk(o):
        if isinstance(o, list):
            return sum(1 for x in o if isinstance(x, (bytes, bytearray)) and len(x) == 64)
        if isinstance(o, tuple):
            return sum(walk(x) for x in o)
        return 0
    return sum(walk(o) for o in ProofStream().deserialize(proof).objects)


def write_golden(directory):
    os.makedirs(directory, exist_ok=True)
    entries = []
    for name, m in FIXTURES:
        stark, proof = prove_seeded(name, m)
        again = prove_seeded(name, m, prepare=lambda s: setattr(s, "native_stages", False))[1]
        assert proof == again, "the two stage drivers disagree on %s %s" % (name, mode_id(m))
        assert make_stark(PROGRAMS[name], m).verify(proof) is True
        if m["grinding_bits"]:
            # tests/test_stark_fri_modes_host.py increments the nonce and expects the proof of work to fail: it must not be a hit by chance
            from stark_brainfuck_amd.fri import check_grinding
            from stark_brainfuck_amd.ip import ProofStream
            ps = ProofStream().deserialize(proof)
            at = next(k for k, obj in enumerate(ps.objects) if type(obj) is int)
            ps.read_index = at
            seed, nonce = ps.verifier_fiat_shamir(), ps.objects[at]
            assert check_grinding(seed, nonce, m["grinding_bits"]) and not check_grinding(seed, nonce + 1, m["grinding_bits"]), \
                "%s %s: nonce %d + 1 is a hit as well; choose other grinding bits for this fixture" % (name, mode_id(m), nonce)
        entry ={"file": fixture_file(name, m), "name": name, "program": PROGRAMS[name], "args": m, "fri_domain_length": stark.fri.domain.length,
                 "proof_len": len(proof), "proof_sha256": hashlib.sha256(proof).hexdigest()}
        with open(os.path.join(directory, entry["file"]), "wb") as f:
            f.write(proof)
        entries.append(entry)
        print("wrote %s  %d bytes  sha256 %s" % (entry["file"], len(proof), entry["proof_sha256"][:16]), flush=True)
    with open(os.path.join(directory, FIXTURE_LIST), "w") as f:
        json.dump({"made_by": "tools/stark_fri_modes.py --write-golden", "randomness": "shake_256(b'bfs-golden-urandom' + name), as tests/test_gpu_stark.py",
                   "proofs": entries}, f, indent=1, sort_keys=True)
        f.write("\n")


def _sync():
    from stark_brainfuck_amd.device import current_stream, synchronize
    synchronize(current_stream())


def time_mode(source, m, reps):
    program, _, _, _, matrices = claim(source)
    prove_ms, verify_ms, proof = [], [], None
    for rep in range(reps + 1):
        stark = make_stark(source, m)
        t0 = time.perf_counter()
        proof = stark.prove(program, *matrices)
        _sync()
        prove_ms.append((time.perf_counter() - t0) * 1e3)
    for rep in range(reps + 1):
        verifier = make_stark(source, m)
        t0 = time.perf_counter()
        verdict = verifier._verify_native(proof)
        verify_ms.append((time.perf_counter() - t0) * 1e3)
        assert verdict is True, "native verify of mode %s: %r" % (mode_id(m), verdict)
    return {"mode": mode_id(m), "args": m, "fri_domain_length": stark.fri.domain.length, "colinearity_checks": stark.num_colinearity_checks,
            "proof_bytes": len(proof), "path_digests": count_digests(proof), "prove_ms": round(statistics.median(prove_ms[1:]), 3),
            "prove_min_ms": round(min(prove_ms[1:]), 3), "verify_ms": round(statistics.median(verify_ms[1:]), 3), "verify_min_ms": round(min(verify_ms[1:]), 3)}


def table(source, label, reps):
    rows = []
    print("%s  (security_level 2 unless the mode says s<level>; g<bits> = grinding)" % label)
    print("  %-14s %6s %12s %13s   %21s   %21s" % ("mode", "checks", "proof bytes", "path digests", "prove median / min ms", "verify median / min ms"))
    for m in TABLE_MODES:
        r = time_mode(source, m, reps)
        rows.append(r)
        print("  %-14s %6d %12d %13d   %10.3f / %-10.3f   %10.3f / %-10.3f" % (r["mode"], r["colinearity_checks"], r["proof_bytes"], r["path_digests"], r["prove_ms"],
                                                                        r["prove_min_ms"], r["verify_ms"], r["verify_min_ms"]), flush=True)
    return rows


def ab_child(reps, package_root):
    """default mode only, for an A/B against another checkout: prove and native verify of "Hello World!" and the 2^11 program"""
    import stark_brainfuck_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(stark_brainfuck_amd.__file__))) == os.path.abspath(package_root or ROOT), stark_brainfuck_amd.__file__
    out = {}
    for label, source in (("hello", HELLO_WORLD), ("loop", PROGRAMS["loop"])):
        from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
        program, running_time, inputs, outputs, matrices = claim(source)
        args = (running_time, len(matrices[1]), program, inputs, outputs)
        prove_ms, verify_ms = [], []
        for rep in range(reps + 2):
            stark = BrainfuckStark(*args)
            t0 = time.perf_counter()
            proof = stark.prove(program, *matrices)
            _sync()
            prove_ms.append((time.perf_counter() - t0) * 1e3)
        for rep in range(reps + 2):
            verifier = BrainfuckStark(*args)
            t0 = time.perf_counter()
            assert verifier.verify(proof) is True
            verify_ms.append((time.perf_counter() - t0) * 1e3)
        out[label] = {"prove_ms": round(statistics.median(prove_ms[2:]), 4), "verify_ms": round(statistics.median(verify_ms[2:]), 4), "proof_bytes": len(proof)}
    print("AB " + json.dumps(out, sort_keys=True))


def ab(parent_root, rounds, reps):
    import subprocess
    series = {"parent": [], "this": []}
    for _ in range(rounds):
        for who, root in (("parent", os.path.abspath(parent_root)), ("this", ROOT)):
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child", "--package-root", root, "--reps", str(reps)],
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            lines = [x for x in res.stdout.splitlines() if x.startswith("AB ")]
            if res.returncode != 0 or not lines:
                raise RuntimeError("%s child failed (exit %d):\n%s" % (who, res.returncode, res.stdout[-2000:]))
            series[who].append(json.loads(lines[0][3:]))
    print("| figure [ms] | parent, per process | this, per process | parent median | this median | parent max - min | verdict |")
    print("|---|---|---|---|---|---|---|")
    for program in ("hello", "loop"):
        for figure in ("prove_ms", "verify_ms"):
            a, b = [r[program][figure] for r in series["parent"]], [r[program][figure] for r in series["this"]]
            ma, mb, spread = statistics.median(a), statistics.median(b), max(a) - min(a)
            print("| %s, `%s` | %s | %s | %.4f | %.4f | %.4f | %s (%+.4f) |" % (program, figure, " ".join("%.4f" % x for x in a), " ".join("%.4f" % x for x in b),
                                                                          ma, mb, spread, "not worse" if mb - ma <= spread else "WORSE", mb - ma), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--package-root", default=None)
    ap.add_argument("--program", default="loop")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--write-golden", default=None)
    ap.add_argument("--ab-child", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.package_root:
        sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is proven here")
    if args.ab_child:
        return ab_child(args.reps, args.package_root)
    if args.ab:
        return ab(args.ab, args.rounds, args.reps)
    if args.write_golden:
        return write_golden(args.write_golden)
    result = {}
    for name in args.program.split(","):
        source = {"hello": HELLO_WORLD, "big": BIG}.get(name, PROGRAMS.get(name, name))
        result[name] = table(source, {"hello": "Hello World!", "big": "nested loops, 37 254 cycles"}.get(name, source), args.reps)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
