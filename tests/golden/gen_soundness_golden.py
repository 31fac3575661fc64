#!/usr/bin/env python3
"""Golden for the REJECTING side of the verifier: what the REFERENCE's BrainfuckStark.verify says

  claims        about the committed proofs stark_<name>_proof.bin when the claim it is asked to check is not the one that was proven
                (another output, input, program word, running time, memory length), and
  false_traces  about proofs its own prover writes, without DEBUG, of the trace of `+.` with ONE CELL changed: the proof's length and
                SHA-256, the number of urandom bytes drawn and the verdict.  No proof bytes are kept.

An outcome is true, false, "assert: <message>" or "error: <exception type>".  The re-implementation's two verifier routes must end in
exactly the recorded outcome, and its two prover paths must write the recorded bytes.

Runs ONLY in the build container (imports /root/reference/code); writes tests/golden/soundness.json.

    python tests/golden/gen_soundness_golden.py                 # both sections; the false traces as parallel processes
    python tests/golden/gen_soundness_golden.py claims          # one section, the other is kept as it is in the file
    python tests/golden/gen_soundness_golden.py false_traces
    python tests/golden/gen_soundness_golden.py case <tag>      # one false trace, printed as a JSON line (what the processes run)
"""
import sys
sys.dont_write_bytecode = True
import contextlib, hashlib, io, json, os, subprocess, time

REF = os.environ.get("BFS_REFERENCE", "/root/reference/code")
sys.path.insert(0, REF)
sys.setrecursionlimit(100000)
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "soundness.json")

PROOFS = ["plus1", "io", "two_io", "loop", "countdown"]
PROGRAM = "+."           # 3 cycles, FRI domain 512: about six minutes of CPython per case
MATRICES = ("processor", "memory", "instruction", "input", "output")
FALSE_TRACES = [
    {"tag": "processor_cell", "matrix": "processor", "row": 1, "column": 5, "add": 1},        # the memory value after `+`
    {"tag": "memory_cell", "matrix": "memory", "row": 1, "column": 2, "add": 5},
    {"tag": "processor_first_row", "matrix": "processor", "row": 0, "column": 0, "add": 1},   # the cycle counter
    {"tag": "instruction_cell", "matrix": "instruction", "row": 2, "column": 1, "add": 1},
    {"tag": "output_cell_honest_claim", "matrix": "output", "row": 0, "column": 0, "add": 1},
    {"tag": "output_cell_matching_claim", "matrix": "output", "row": 0, "column": 0, "add": 1, "claimed_output_add": 1},
]


class Stream:
    """the urandom of gen_debug_golden.py / gen_stark_golden.py"""

    def __init__(self, tag):
        self.tag, self.pos, self.buf = tag, 0, b""

    def __call__(self, n):
        end = self.pos + n
        if end > len(self.buf):
            self.buf = hashlib.shake_256(b"bfs-golden-urandom" + self.tag).digest(max(2 * end, 1 << 16))
        out = self.buf[self.pos:end]
        self.pos = end
        return out


def outcome_of(call):
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            value = call()
        assert value is True or value is False, value
        return value
    except AssertionError as e:
        return "assert: " + str(e)
    except Exception as e:          # noqa: BLE001 -- whatever the reference raises is the record
        return "error: " + type(e).__name__


def altered_claims(running_time, memory_length, words, inputs, outputs):
    """[(tag, (running_time, memory_length, program words, input symbols, output symbols))]: each only where there is such a symbol"""
    def bump(symbols, k):
        return symbols[:k] + [chr(ord(symbols[k]) + 1)] + symbols[k + 1:]
    out = [("honest", (running_time, memory_length, words, inputs, outputs)),
           ("output_appended", (running_time, memory_length, words, inputs, outputs + ["!"]))]
    if outputs:
        out.append(("output_changed", (running_time, memory_length, words, inputs, bump(outputs, len(outputs) // 2))))
        out.append(("output_dropped", (running_time, memory_length, words, inputs, outputs[:-1])))
    out.append(("input_appended", (running_time, memory_length, words, inputs + ["!"], outputs)))
    if inputs:
        out.append(("input_changed", (running_time, memory_length, words, bump(inputs, 0), outputs)))
    k = len(words) // 2
    out.append(("program_word_changed", (running_time, memory_length, words[:k] + [words[k] + 1] + words[k + 1:], inputs, outputs)))
    out.append(("running_time_plus_1", (running_time + 1, memory_length, words, inputs, outputs)))
    out.append(("running_time_minus_1", (running_time - 1, memory_length, words, inputs, outputs)))
    out.append(("running_time_doubled", (2 * running_time, memory_length, words, inputs, outputs)))
    out.append(("memory_length_plus_1", (running_time, memory_length + 1, words, inputs, outputs)))
    return out


def claims():
    import brainfuck_stark as bs
    from algebra import BaseFieldElement
    from vm import VirtualMachine
    field = VirtualMachine.field
    section = {}
    for name in PROOFS:
        g = json.load(open(os.path.join(HERE, "stark_%s.json" % name)))
        proof = open(os.path.join(HERE, "stark_%s_proof.bin" % name), "rb").read()
        assert hashlib.sha256(proof).hexdigest() == g["proof_sha256"]
        program = VirtualMachine.compile(g["program"])
        running_time, input_symbols, output_symbols = VirtualMachine.run(program, input_data=list(g["input"]))
        assert running_time == g["running_time"] and [e.value for e in program] == g["compiled_program"]
        words = [e.value for e in program]
        entries = []
        for tag, (rt, ml, ws, ins, outs) in altered_claims(running_time, g["matrix_shapes"]["memory"][0], words, list(input_symbols), list(output_symbols)):
            t0 = time.time()
            verdict = outcome_of(lambda: bs.BrainfuckStark(rt, ml, [BaseFieldElement(w, field) for w in ws], ins, outs).verify(proof))
            entries.append({"tag": tag, "running_time": rt, "memory_length": ml, "program": ws, "input": "".join(ins), "output": "".join(outs),
                            "outcome": verdict, "seconds": round(time.time() - t0, 1)})
            print(name, json.dumps(entries[-1]), flush=True)
        assert entries[0]["outcome"] is True
        section[name] = entries
    return section


def false_trace(tag):
    case = next(c for c in FALSE_TRACES if c["tag"] == tag)
    os.environ.pop("DEBUG", None)
    stream = Stream(("soundness-" + tag).encode())
    os.urandom = stream
    import salted_merkle
    salted_merkle.urandom = stream
    import brainfuck_stark as bs
    from vm import VirtualMachine
    program = VirtualMachine.compile(PROGRAM)
    running_time, input_symbols, output_symbols = VirtualMachine.run(program, input_data=[])
    matrices = dict(zip(MATRICES, VirtualMachine.simulate(program, input_data=list(input_symbols))))
    m = matrices[case["matrix"]]
    cell = m[case["row"]][case["column"]]
    out = dict(case)
    out["shapes"] = {k: [len(mx), len(mx[0]) if mx else 0] for k, mx in matrices.items()}
    out["honest_value"] = cell.value
    m[case["row"]][case["column"]] = cell + type(cell)(case["add"], cell.field)
    claimed = [chr(ord(o) + case.get("claimed_output_add", 0)) for o in output_symbols]
    out["claimed_output"] = "".join(claimed)
    args = (running_time, len(matrices["memory"]), program, list(input_symbols), claimed)
    out["running_time"], out["memory_length"] = args[0], args[1]
    stark = bs.BrainfuckStark(*args)
    out["fri_domain_length"], out["max_degree"] = stark.fri.domain.length, stark.max_degree
    t0 = time.time()
    with contextlib.redirect_stdout(io.StringIO()):
        proof = stark.prove(program, *(matrices[k] for k in MATRICES))
    out["prove_seconds"] = round(time.time() - t0, 1)
    out["proof_len"], out["proof_sha256"], out["urandom_bytes"] = len(proof), hashlib.sha256(proof).hexdigest(), stream.pos
    t0 = time.time()
    out["outcome"] = outcome_of(lambda: bs.BrainfuckStark(*args).verify(proof))          # a verifier that has seen nothing but claim and proof
    out["verify_seconds"] = round(time.time() - t0, 1)
    out["outcome_on_the_provers_instance"] = outcome_of(lambda: stark.verify(proof))
    return out


def false_traces():
    t0 = time.time()
    children = [(c["tag"], subprocess.Popen([sys.executable, os.path.abspath(__file__), "case", c["tag"]], stdout=subprocess.PIPE, text=True))
                for c in FALSE_TRACES]
    cases = []
    for tag, child in children:
        text, _ = child.communicate()
        assert child.returncode == 0, (tag, child.returncode)
        cases.append(json.loads(text.strip().splitlines()[-1]))
        print(json.dumps(cases[-1]), flush=True)
    return {"program": PROGRAM, "urandom": "SHAKE-256('bfs-golden-urandom' || 'soundness-' || tag)", "processes": len(children),
            "wall_seconds": round(time.time() - t0, 1), "cases": cases}


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what == "case":
        print(json.dumps(false_trace(sys.argv[2])), flush=True)
        return
    rec = json.load(open(OUT)) if os.path.exists(OUT) else {}
    if what in ("all", "false_traces"):
        rec["false_traces"] = false_traces()
    if what in ("all", "claims"):
        t0 = time.time()
        rec["claims"] = claims()
        rec["claims_seconds"] = round(time.time() - t0, 1)
    with open(OUT, "w") as f:
        json.dump({k: rec[k] for k in sorted(rec)}, f, indent=1)


if __name__ == "__main__":
    main()
