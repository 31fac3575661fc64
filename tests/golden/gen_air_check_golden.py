#!/usr/bin/env python3
"""Golden for the trace checker (Table.test / Table.xtest, table.py:48-110): runs the REFERENCE's checks on small traces -- as the VM
wrote them, padded, and with single corrupted cells -- and records its verdicts: "pass", the (kind, constraint index, row) of the first
failure, or "error: ..." when it stops for a reason that is not the AIR.  Also records each table's base constraint counts and the
values of its base_*_constraints() at seeded random points.  The re-implementation (Table.test / xtest / air_violations) must agree.

Runs ONLY in the build container (imports /root/reference/code); needs no proving; writes tests/golden/air_check.json.

    python tests/golden/gen_air_check_golden.py
"""
import sys
sys.dont_write_bytecode = True
import contextlib, io, json, os, random, re, traceback

REF = os.environ.get("BFS_REFERENCE", "/root/reference/code")
sys.path.insert(0, REF)
sys.setrecursionlimit(100000)
HERE = os.path.dirname(os.path.abspath(__file__))
P = (1 << 64) - (1 << 32) + 1

PROGRAMS = [          # (code, input)
    ("++[>+++<-]>.", ""),
    (",+.,-.", "ab"),                # input and output
    ("+[-]>++<", ""),                # empty input and output
    ("-+>-<[>+<+]>++.", ""),         # memory values next to p
]
TABLES = ["processor", "instruction", "memory", "input", "output"]
# (program index, table, row ("first" / "middle" / "last"), column, added value)
CORRUPTIONS = [(0, "processor", "first", 0, 1), (0, "processor", "middle", 5, 1), (0, "processor", "last", 1, 1),
               (1, "processor", "middle", 2, 1), (2, "processor", "middle", 6, 3), (3, "processor", "last", 5, P - 1),
               (0, "instruction", "first", 0, 1), (0, "instruction", "middle", 1, 1), (1, "instruction", "last", 2, 1),
               (0, "memory", "first", 2, 1), (1, "memory", "middle", 0, 1), (3, "memory", "last", 1, 1),
               (2, "memory", "middle", 3, 1)]
# xtest corruptions on padded, extended tables: (program index, table, row, column (full width), added value)
X_CORRUPTIONS = [(0, "processor", "middle", 1, 1), (0, "processor", "last", 8, 1), (1, "processor", "middle", 9, 1),
                 (0, "instruction", "middle", 3, 1), (1, "instruction", "first", 4, 1), (0, "memory", "middle", 4, 1),
                 (1, "input", "first", 1, 1), (1, "output", "last", 0, 1), (2, "memory", "last", 2, 1)]


def pick(rows, where):
    return {"first": 0, "middle": rows // 2, "last": rows - 1}[where]


def verdict_of_test(fn):
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            fn()
        return "pass"
    except AssertionError as e:
        msg = str(e)
        m = re.match(r"BOUNDARY constraint (\d+) not satisfied", msg)
        if m:
            return ["boundary", int(m.group(1)), 0]
        m = re.match(r"TRNASITION constraint (\d+) not satisfied in row (\d+)", msg)
        if m:
            return ["transition", int(m.group(1)), int(m.group(2))]
        return "error: AssertionError: " + msg.splitlines()[0][:200] if msg else "error: AssertionError"
    except Exception as e:
        return "error: %s: %s" % (type(e).__name__, str(e).splitlines()[0][:200] if str(e) else "")


def verdict_of_xtest(table, challenges, terminals):
    """Table.xtest asserts without a message: the kind comes from the line that raised, the index and row from the loop variables"""
    import table as ref_table
    src = open(ref_table.__file__).read().splitlines()
    start = next(k for k, l in enumerate(src) if "def xtest" in l) + 1
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            table.xtest(challenges, terminals)
        return "pass"
    except Exception as exc:
        tb = sys.exc_info()[2]
        frame = None
        while tb is not None:
            if tb.tb_frame.f_code.co_name == "xtest":
                frame, line = tb.tb_frame, tb.tb_lineno
            tb = tb.tb_next
        if frame is None:
            return "error: %s: %s" % (type(exc).__name__, str(exc).splitlines()[0][:200] if str(exc) else "")
        section = [l for l in src[start - 1:line] if l.strip().startswith("# test ")][-1]
        kind = section.strip().split()[2]
        i = frame.f_locals["i"]
        if kind == "terminal":
            # a failing terminal constraint prints diagnostics first, and for tables without `terminal_index` (processor, instruction,
            # memory) that print raises AttributeError: either way the constraint failed
            return ["terminal", i, table.height - 1]
        if not isinstance(exc, AssertionError):
            return "error: %s: %s" % (type(exc).__name__, str(exc).splitlines()[0][:200] if str(exc) else "")
        if kind == "boundary":
            return ["boundary", i, 0]
        return ["transition", i, frame.f_locals["j"]]


def ints(row):
    out = []
    for v in row:
        if hasattr(v, "polynomial"):
            cs = [c.value for c in v.polynomial.coefficients] + [0, 0, 0]
            out.append(cs[:3])
        else:
            out.append(v.value)
    return out


def main():
    from algebra import BaseFieldElement
    from brainfuck_stark import BrainfuckStark
    from extension_field import ExtensionFieldElement
    from univariate import Polynomial
    from vm import VirtualMachine
    field, xfield = BrainfuckStark.field, BrainfuckStark.xfield

    def xe(t):
        return ExtensionFieldElement(Polynomial([BaseFieldElement(v, field) for v in t]), xfield)

    rng = random.Random(0xC4EC)
    rec = {"constraints": {}, "programs": [], "xtest": {}}

    def setup(code, inp):
        program = VirtualMachine.compile(code)
        running_time, input_symbols, output_symbols = VirtualMachine.run(program, input_data=list(inp))
        matrices = VirtualMachine.simulate(program, input_data=list(input_symbols))
        pm, mm, im, inm, om = matrices
        stark = BrainfuckStark(running_time, len(mm), program, input_symbols, output_symbols)
        tables = dict(zip(TABLES, stark.tables))
        for name, m in zip(["processor", "memory", "instruction", "input", "output"], matrices):
            tables[name].matrix = [list(r) for r in m]
        return stark, tables, input_symbols, output_symbols

    # base constraint sets: counts, and values at random points
    stark, tables, _, _ = setup(*PROGRAMS[0])
    for name in TABLES:
        t = tables[name]
        bcs, tcs = t.base_boundary_constraints(), t.base_transition_constraints()
        entry = {"counts": [len(bcs), len(tcs)], "boundary_values": [], "transition_values": []}
        for _ in range(3):
            pt = [rng.randrange(P) for _ in range(t.base_width)]
            entry["boundary_values"].append([pt, [c.evaluate([BaseFieldElement(v, field) for v in pt]).value for c in bcs]])
            pt = [rng.randrange(P) for _ in range(2 * t.base_width)]
            if name == "processor":
                pt[2] = ord("+-<>[],."[rng.randrange(8)])        # a real instruction in the current-instruction column
            entry["transition_values"].append([pt, [c.evaluate([BaseFieldElement(v, field) for v in pt]).value for c in tcs]])
        rec["constraints"][name] = entry

    # Table.test verdicts
    for pi, (code, inp) in enumerate(PROGRAMS):
        entry = {"code": code, "input": inp, "unpadded": {}, "padded": {}, "corruptions": []}
        stark, tables, _, _ = setup(code, inp)
        entry["lengths"] = {n: len(tables[n].matrix) for n in TABLES}
        for name in TABLES:
            entry["unpadded"][name] = verdict_of_test(tables[name].test)
        for name in TABLES:
            stark2, tables2, _, _ = setup(code, inp)
            t = tables2[name]
            try:
                t.pad()
                entry["padded"][name] = verdict_of_test(t.test)
            except Exception as e:
                entry["padded"][name] = "error: %s: %s" % (type(e).__name__, str(e)[:200])
        for (k, name, where, col, add) in CORRUPTIONS:
            if k != pi:
                continue
            stark, tables, _, _ = setup(code, inp)
            t = tables[name]
            row = pick(len(t.matrix), where)
            t.matrix[row][col] = t.matrix[row][col] + BaseFieldElement(add, field)
            entry["corruptions"].append({"table": name, "row": row, "column": col, "add": add, "verdict": verdict_of_test(t.test)})
        rec["programs"].append(entry)
        print(code, entry["unpadded"], entry["padded"], [c["verdict"] for c in entry["corruptions"]], flush=True)

    # Table.xtest verdicts on padded, extended tables (brainfuck_stark.py:134-190), fixed challenges and initials
    challenges = [[rng.randrange(P) for _ in range(3)] for _ in range(11)]
    initials = [[rng.randrange(P) for _ in range(3)] for _ in range(2)]
    rec["xtest"] = {"challenges": challenges, "initials": initials, "programs": []}
    for pi, (code, inp) in enumerate(PROGRAMS):
        cases = [None] + [c for c in X_CORRUPTIONS if c[0] == pi]
        out = {"code": code, "input": inp, "clean": None, "corruptions": []}
        for case in cases:
            stark, tables, _, _ = setup(code, inp)
            for name in ("processor", "memory", "instruction", "input", "output"):
                tables[name].pad()
            ch, it = [xe(c) for c in challenges], [xe(c) for c in initials]
            for t in stark.tables:
                t.codewords = []             # (extend lifts the codewords of lde(), which the checks do not need)
                t.extend(ch, it)
            terminals = stark.get_terminals()
            if case is None:
                out["clean"] = {n: verdict_of_xtest(tables[n], ch, terminals) for n in TABLES}
                out["terminals"] = [ints([tm])[0] for tm in terminals]
                continue
            _, name, where, col, add = case
            t = tables[name]
            row = pick(t.height, where)
            cell = t.matrix[row][col]
            t.matrix[row][col] = cell + (xfield(add) if hasattr(cell, "polynomial") else BaseFieldElement(add, field))
            out["corruptions"].append({"table": name, "row": row, "column": col, "add": add,
                                       "verdict": verdict_of_xtest(t, ch, terminals)})
        rec["xtest"]["programs"].append(out)
        print("xtest", code, out["clean"], [c["verdict"] for c in out["corruptions"]], flush=True)

    with open(os.path.join(HERE, "air_check.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
