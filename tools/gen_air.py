#!/usr/bin/env python3
"""Generates stark_brainfuck_amd/csrc/air_generated.hpp from the constraint graphs in stark_brainfuck_amd/air.py:
one straight-line device function per table that evaluates every boundary / transition / terminal constraint at
one point of the FRI domain ("needs the constraint polynomials hard-coded").  Also generates
csrc/air_base_generated.hpp: the same for the BASE AIR (TableAir.base(), what Table.test() checks on a base trace).

Base columns stay single 64-bit residues until they meet an extension value (challenge, terminal, extension
column); common subexpressions (deselectors, instruction zerofiers, differences of neighbouring rows) are shared.

    python tools/gen_air.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import importlib.util

spec = importlib.util.spec_from_file_location("air", os.path.join(ROOT, "stark_brainfuck_amd", "air.py"))
air = importlib.util.module_from_spec(spec)
spec.loader.exec_module(air)

OUT = os.path.join(ROOT, "stark_brainfuck_amd", "csrc", "air_generated.hpp")
OUT_BASE = os.path.join(ROOT, "stark_brainfuck_amd", "csrc", "air_base_generated.hpp")


class Gen:
    def __init__(self, base_width):
        self.base_width = base_width
        self.table = {}      # structural key -> (name, is_ext)
        self.lines = []
        self.count = 0
        self.by_id = {}
        self.n_base_ops = self.n_ext_ops = 0

    def emit(self, e):
        if id(e) in self.by_id:
            return self.by_id[id(e)]
        op = e.op
        if op == "v":
            col, nxt = e.val
            if col < self.base_width:
                r = ("%s[%d]" % ("bn" if nxt else "bc", col), False)
            else:
                r = ("%s[%d]" % ("xn" if nxt else "xc", col - self.base_width), True)
        elif op == "k":
            r = ("%dULL" % e.val, False)
        elif op == "c":
            r = ("ch[%d]" % e.val, True)
        elif op == "t":
            r = ("tm[%d]" % e.val, True)
        elif op == "p":
            r = ("pr[%d]" % e.val, True)
        else:
            a = self.emit(e.a)
            b = self.emit(e.b) if e.b is not None else None
            key = (op, a[0], b[0] if b else None)
            if op in "+*" and b is not None and b[0] < a[0]:
                key = (op, b[0], a[0])               # commutative: one canonical order
            if key in self.table:
                r = self.table[key]
            else:
                r = self.compute(op, a, b)
                self.table[key] = r
        self.by_id[id(e)] = r
        return r

    def new(self, is_ext, expr):
        name = "t%d" % self.count
        self.count += 1
        self.lines.append("    const %s %s = %s;" % ("Xfe" if is_ext else "u64", name, expr))
        if is_ext:
            self.n_ext_ops += 1
        else:
            self.n_base_ops += 1
        return (name, is_ext)

    def compute(self, op, a, b):
        if op == "n":
            return self.new(a[1], ("xfe_neg(%s)" if a[1] else "gl_neg(%s)") % a[0])
        (an, ax), (bn, bx) = a, b
        if not ax and not bx:
            if op == "*" and an == "1ULL":
                return b
            if op == "*" and bn == "1ULL":
                return a
            return self.new(False, "%s(%s, %s)" % ({"+": "gl_add", "-": "gl_sub", "*": "gl_mul"}[op], an, bn))
        if ax and bx:
            return self.new(True, "%s(%s, %s)" % ({"+": "xfe_add", "-": "xfe_sub", "*": "xfe_mul"}[op], an, bn))
        if op == "*":
            x, s = (an, bn) if ax else (bn, an)
            if s == "1ULL":
                return (x, True)
            return self.new(True, "xfe_scale(%s, %s)" % (x, s))
        if op == "+":
            x, s = (an, bn) if ax else (bn, an)
            return self.new(True, "xfe_add_base(%s, %s)" % (x, s))
        if ax:                       # ext - base
            return self.new(True, "xfe_sub_base(%s, %s)" % (an, bn))
        return self.new(True, "xfe_base_sub(%s, %s)" % (an, bn))    # base - ext


def generic_degrees(ta):
    """total degree of every constraint's exact expansion for challenges / terminals / parameters that look sampled"""
    import random
    rng = random.Random(0xA1B)
    p = (1 << 64) - (1 << 32) + 1
    ch = [tuple(rng.randrange(1 << 33, p) for _ in range(3)) for _ in range(11)]
    tm = [tuple(rng.randrange(1 << 33, p) for _ in range(3)) for _ in range(5)]
    pr = [tuple(rng.randrange(1 << 33, p) for _ in range(3)) for _ in range(max(ta.num_params, 1))]
    out = []
    for kind, cons in ta.all():
        nvars = 2 * ta.full_width if kind == "transition" else ta.full_width
        memo = {}
        for e in cons:
            out.append(max([0] + list(air.total_degrees(air.expand(e, nvars, ch, tm if kind == "terminal" else [air.X0] * 5, pr, memo)))))
    return out


def write_if_changed(path, text):
    if os.path.exists(path) and open(path).read() == text:
        print("unchanged", path)          # keep the file's time stamp: the library build compares it with the .so
    else:
        with open(path, "w") as f:
            f.write(text)
        print("wrote", path)


def main_base():
    """air_base_generated.hpp: per table air_<table>_base(bc, bn, sink), base constraints only (boundary, then transition)"""
    out = ["// air_base_generated.hpp -- GENERATED by tools/gen_air.py from stark_brainfuck_amd/air.py, do not edit.",
           "// The BASE constraint polynomials of the five tables (TableAir.base_boundary / base_transition: the reference's",
           "// base_boundary_constraints / base_transition_constraints) evaluated at one point (current row, next row) of a base trace.",
           "// Values are handed to the sink as they are computed (`put_base<index>(value)`, boundary first, then transition).",
           "#pragma once", '#include "gl.hpp"', "", "namespace bfs {", "namespace airgen {", "",
           "struct BaseArraySink {", "    u64* out;", "    template <int I> BFS_HD void put_base(u64 v) { out[I] = v; }", "};", ""]
    for ta in air.TABLE_AIRS:
        g = Gen(ta.base_width)
        body, n = [], 0
        counts = []
        for kind, cons in ta.base():
            counts.append(len(cons))
            for e in cons:
                name, is_ext = g.emit(e)
                assert not is_ext, "a base constraint reads an extension operand"
                body.extend(g.lines)
                g.lines = []
                body.append("    sink.template put_base<%d>(%s);" % (n, name))
                n += 1
        up = ta.name.upper()
        out.append("// %s table: %d base boundary, %d base transition constraints; %d operations" % (ta.name, counts[0], counts[1], g.n_base_ops))
        out.append("constexpr int %s_BASE_NUM_BOUNDARY = %d, %s_BASE_NUM_TRANSITION = %d;" % (up, counts[0], up, counts[1]))
        out.append("template <class Sink, class BN = const u64*>")
        out.append("BFS_HD void air_%s_base(const u64* bc, BN bn, Sink& sink) {" % ta.name)
        if not body:
            out.append("    (void)bc; (void)bn; (void)sink;")
        out.extend(body)
        out.append("}")
        out.append("BFS_HD void air_%s_base_values(const u64* bc, const u64* bn, u64* out) {" % ta.name)
        out.append("    BaseArraySink sink{out};")
        out.append("    air_%s_base(bc, bn, sink);" % ta.name)
        out.append("}")
        out.append("")
    out += ["}  // namespace airgen", "}  // namespace bfs", ""]
    write_if_changed(OUT_BASE, "\n".join(out))


def main():
    out = ["// air_generated.hpp -- GENERATED by tools/gen_air.py from stark_brainfuck_amd/air.py, do not edit.",
           "// Constraint polynomials of the five tables evaluated at one point (current row, next row); replaces the symbolic",
           "// MPolynomial.evaluate of /root/reference/code/table.py:163-164,207-211,255-256.  Results are written in the order",
           "// boundary, transition, terminal (table.py:274-281).",
           "#pragma once", '#include "gl.hpp"', "", "namespace bfs {", "namespace airgen {", ""]
    counts = []
    out += ["// A sink receives every constraint value as soon as it is computed (`put<index>(value)`, in the order boundary, transition,",
            "// terminal): the quotient kernels scale and store or accumulate it at once instead of keeping all of them in registers.",
            "struct ArraySink {", "    Xfe* out;", "    template <int I> BFS_HD void put(const Xfe& v) { out[I] = v; }",
            "    template <int I> BFS_HD void put_base(u64 v) { out[I] = xfe_lift(v); }      // a constraint without extension operands", "};", ""]
    for ta in air.TABLE_AIRS:
        g = Gen(ta.base_width)
        kinds = []
        body = []
        for kind, cons in ta.all():
            for e in cons:
                name, is_ext = g.emit(e)
                body.extend(g.lines)
                g.lines = []
                body.append("    sink.template %s<%d>(%s);" % ("put" if is_ext else "put_base", len(kinds), name))
                kinds.append(kind)
        is_ext_flags = [("put<" in l) for l in body if "sink.template" in l]
        nb = sum(1 for k in kinds if k == "boundary")
        nt = sum(1 for k in kinds if k == "transition")
        nz = sum(1 for k in kinds if k == "terminal")
        counts.append((ta.name, nb, nt, nz, g.n_base_ops, g.n_ext_ops))
        out.append("// %s table: %d boundary, %d transition, %d terminal constraints; %d base and %d extension operations"
                   % (ta.name, nb, nt, nz, g.n_base_ops, g.n_ext_ops))
        out.append("constexpr int %s_BASE_WIDTH = %d, %s_EXT_WIDTH = %d, %s_NUM_BOUNDARY = %d, %s_NUM_TRANSITION = %d, %s_NUM_TERMINAL = %d;"
                   % (ta.name.upper(), ta.base_width, ta.name.upper(), ta.full_width - ta.base_width, ta.name.upper(), nb,
                      ta.name.upper(), nt, ta.name.upper(), nz))
        # what the combination's sink needs to know at compile time about quotient q: does the generated code hand over an extension
        # value (put) or a base value (put_base), and the GENERIC total degree of the constraint (for sampled challenges; the degree
        # bound is that times the interpolant degree minus the zerofier's, table.py:170-173) -- neighbouring quotients of one kind
        # with equal degrees normally share their shift, which lets the sink apply x^shift once per run (the launcher checks the
        # actual shifts and falls back to one run per term when they differ)
        out.append("constexpr bool %s_Q_EXT[] = {%s};" % (ta.name.upper(), ", ".join("true" if f else "false" for f in is_ext_flags)))
        out.append("constexpr unsigned char %s_Q_DEGREE[] = {%s};" % (ta.name.upper(), ", ".join(str(d) for d in generic_degrees(ta))))
        # bn / xn (the NEXT row) are anything indexable: plain arrays, or accessors that fetch from LDS at the point of use
        out.append("template <class Sink, class BN = const u64*, class XN = const Xfe*>")
        out.append("BFS_HD void air_%s(const u64* bc, BN bn, const Xfe* xc, XN xn, const Xfe* ch, const Xfe* tm, const Xfe* pr, Sink& sink) {" % ta.name)
        out.extend(body)
        out.append("}")
        out.append("BFS_HD void air_%s_values(const u64* bc, const u64* bn, const Xfe* xc, const Xfe* xn, const Xfe* ch, const Xfe* tm, const Xfe* pr, Xfe* out) {" % ta.name)
        out.append("    ArraySink sink{out};")
        out.append("    air_%s(bc, bn, xc, xn, ch, tm, pr, sink);" % ta.name)
        out.append("}")
        out.append("")
    out += ["}  // namespace airgen", "}  // namespace bfs", ""]
    write_if_changed(OUT, "\n".join(out))
    for c in counts:
        print("  %-12s boundary %d transition %d terminal %d | base ops %d, extension ops %d" % c)


if __name__ == "__main__":
    main()
    main_base()
