#!/usr/bin/env python3
"""Golden for the extension stage: runs the REFERENCE's `extend` (processor_table.py:359-427, instruction_table.py:171-231,
memory_table.py:174-206, io_table.py:77-110) on every synthetic table of tests/extend_cases.py and records, per case and extension
column, the SHA-256 of the column (row after row the three limbs as little-endian 64-bit words), the limb triples at rows 0, 1,
254 .. 257 and the last two rows, and the terminals the reference leaves on the table object.  tests/test_extend_host.py holds the
plain-integer restatement tests/extend_model.py against it.

Runs ONLY in the build container (imports /root/reference/code); a few seconds; writes tests/golden/extend.json.

    python tests/golden/gen_extend_golden.py
"""
import sys
sys.dont_write_bytecode = True
import hashlib, json, os, struct

REF = os.environ.get("BFS_REFERENCE", "/root/reference/code")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(1, os.path.dirname(HERE))           # tests/: extend_cases, field_states, scan_model (no name of theirs is the reference's)

TERMINALS = {"processor": ["instruction_permutation_terminal", "memory_permutation_terminal", "input_evaluation_terminal", "output_evaluation_terminal"],
             "instruction": ["permutation_terminal", "evaluation_terminal"], "memory": ["permutation_terminal"],
             "input": ["evaluation_terminal"], "output": ["evaluation_terminal"]}


def limbs(v):
    cs = [c.value for c in v.polynomial.coefficients] + [0, 0, 0]
    assert not any(cs[3:]) and all(0 <= c < (1 << 64) - (1 << 32) + 1 for c in cs[:3])
    return cs[:3]


def main():
    import extend_cases
    from algebra import BaseFieldElement
    from brainfuck_stark import BrainfuckStark
    from extension_field import ExtensionFieldElement
    from instruction_table import InstructionTable
    from io_table import InputTable, OutputTable
    from memory_table import MemoryTable
    from processor_table import ProcessorTable
    from univariate import Polynomial
    field, xfield = BrainfuckStark.field, BrainfuckStark.xfield
    generator, order = field.generator(), 1 << 32

    def xe(t):
        return ExtensionFieldElement(Polynomial([BaseFieldElement(v, field) for v in t]), xfield)

    def make(case):
        name, h = case["table"], case["height"]
        if name in ("input", "output"):
            t = (InputTable if name == "input" else OutputTable)(field, h, generator, order)
            t.length, t.height = case["length"], h
        else:
            t = {"processor": ProcessorTable, "instruction": InstructionTable, "memory": MemoryTable}[name](field, h, 1, generator, order)
        t.matrix = [[BaseFieldElement(v, field) for v in row] for row in case["matrix"]]
        t.codewords = []                   # (extend lifts the codewords of lde(), which nothing here needs)
        return t

    rec = {}
    for case in extend_cases.all_cases():
        t = make(case)
        base_width = len(case["matrix"][0])
        t.extend([xe(c) for c in case["challenges"]], [xe(c) for c in case["initials"]])
        assert len(t.matrix) == case["height"]
        rows = extend_cases.sample_rows(case["height"])
        columns = []
        for k in range(extend_cases.EXT_WIDTH[case["table"]]):
            col = [limbs(row[base_width + k]) for row in t.matrix]
            digest = hashlib.sha256(b"".join(struct.pack("<3Q", *v) for v in col)).hexdigest()
            columns.append({"sha256": digest, "samples": [[i] + col[i] for i in rows]})
        rec[case["name"]] = {"height": case["height"], "columns": columns,
                             "terminals": [limbs(getattr(t, attr)) for attr in TERMINALS[case["table"]]]}
        print(case["name"], [c["sha256"][:12] for c in columns], flush=True)
    with open(os.path.join(HERE, "extend.json"), "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in rec.items()) + "\n}\n")


if __name__ == "__main__":
    main()
