"""Synthetic padded tables for the extension stage, built from a seeded rule that the fixture's generator (golden/gen_extend_golden.py)
and the tests share.  No test lives here and nothing here calls the package.

A GROUP is one set of challenges and initials with one table of each kind, so that a group can go through one call that extends all
five tables; `cases(table)` lists that table's case of every group.  Cells are canonical (< p).

  fill      "cycle": palette values (field_states.PALETTE) cycling down the rows, another phase in every column; "constant": one
            palette value everywhere; "random": random residues
  ch        challenges and initials with limbs drawn from the palette, random ones, or "zero_evals": eta = gamma = delta = 0
  control   the columns the loops branch on are then overwritten so that every branch occurs (patterns below): the processor's
            current instruction (0, ',', '.', others), the instruction table's addresses (repeated / changing) and current
            instruction (0 / not), the memory table's dummy flag (0 / 1).  "edges" and "dense" force update rows at 0, 255, 256 and 511
            (both ends of both workgroups of a 512-row scan), "gap" / "long_same" / "long_changing" hold a run of more than 256 rows
            that an extension column does not absorb.  ',' never stands on the last processor row: the reference reads the next row there.
  zero      the group "zero": alpha and beta are solved so that the factor of one product row is exactly zero -- processor row 300 (the
            middle of a workgroup), instruction row 256 and memory row 255 (workgroup edges) carry that row's cells -- and every later
            state of the three permutation products is 0

row0_case() is apart from the groups: a tiny instruction table whose first address is p - 1, the value the reference's loop starts its
`previous_address` with (instruction_table.py:184), so that row 0 does NOT enter the running evaluation.  No group has such a row 0."""
import random

from field_states import PALETTE
from scan_model import P, X0, xadd, xscale

TABLES = ("processor", "instruction", "memory", "input", "output")
WIDTH = {"processor": 7, "instruction": 3, "memory": 4, "input": 1, "output": 1}
EXT_WIDTH = {"processor": 4, "instruction": 2, "memory": 1, "input": 1, "output": 1}
COMMA, DOT, PLUS, OPEN = ord(","), ord("."), ord("+"), ord("[")
EDGE_ROWS = (0, 255, 256, 511)
GAP = range(120, 401)                # 281 rows

# name, height, fill, challenges, control pattern of processor / instruction / memory, lengths of input / output
GROUPS = (
    ("cycle", 512, "cycle", "palette", "edges", "edges", "edges", 512, 300),
    ("constant", 512, "constant", "palette", "dense", "constant", "dense", 1, 512),
    ("random", 512, "random", "random", "gap", "long_same", "gap", 257, 256),
    ("changing", 512, "random", "palette", "dense", "long_changing", "dense", 512, 511),
    ("zero", 512, "random", "random", "dense", "runs", "dense", 255, 2),
    ("zero_evals", 512, "cycle", "zero_evals", "dense", "runs", "gap", 512, 512),
    ("one_row", 1, "random", "random", "dense", "runs", "dense", 1, 1),
    ("two_rows", 2, "cycle", "palette", "edges", "runs", "dense", 2, 1),
    ("two_rows_random", 2, "random", "random", "dense", "constant", "edges", 1, 2),
)
ZERO_ROWS = {"processor": 300, "instruction": 256, "memory": 255}


def _fill(rng, fill, width, height, phase):
    if fill == "cycle":
        return [[PALETTE[(i + 4 * c + phase) % len(PALETTE)] for c in range(width)] for i in range(height)]
    if fill == "constant":
        v = PALETTE[phase % len(PALETTE)]
        return [[v] * width for _ in range(height)]
    return [[rng.randrange(P) for _ in range(width)] for _ in range(height)]


def _element(rng, mode):
    if mode == "random":
        return tuple(rng.randrange(P) for _ in range(3))
    return tuple(rng.choice(PALETTE) for _ in range(3))


def _processor_control(rng, m, pattern):
    h = len(m)
    if pattern == "edges":
        forced = {0: COMMA, 1: DOT, 254: PLUS, 255: DOT, 256: COMMA, 257: OPEN, 510: COMMA, 511: DOT}
        ci = [0] * h
    else:
        forced = {0: DOT, 255: COMMA, 256: DOT, 511: PLUS}
        ci = [rng.choice((0, 0, COMMA, DOT, PLUS, OPEN, 1, P - 1)) for _ in range(h)]
        if pattern == "gap":
            forced = {0: DOT, 511: PLUS}
            for i in GAP:
                ci[i] = 0
    for i, v in forced.items():
        if i < h:
            ci[i] = v
    if ci[h - 1] == COMMA:
        ci[h - 1] = DOT
    for i in range(h):
        m[i][2] = ci[i]


def _instruction_control(rng, m, fill, pattern):
    h = len(m)
    for i in range(h):
        m[i][1] = rng.choice((0, m[i][1], m[i][1], PLUS)) if pattern != "edges" else (0 if i % 3 == 0 else m[i][1] or 1)
    if pattern == "constant":            # the addresses stay as the fill made them
        if m[0][0] == P - 1:
            for i in range(h):
                m[i][0] = P - 2
        return
    drawn = [0]

    def fresh(previous):
        while True:
            drawn[0] += 1
            v = rng.randrange(P) if fill == "random" else PALETTE[drawn[0] % len(PALETTE)]
            if v != previous and v != P - 1:
                return v
    if pattern == "edges":               # the address changes exactly at rows 255, 256 and 511
        starts = {0, 255, 256, 511}
    else:
        starts, i = set(), 0
        while i < h:
            starts.add(i)
            i += rng.randrange(1, 5)
        starts -= {255, 256, 511}        # these rows repeat the address above them: rows of the product
        if pattern == "long_same":
            starts -= set(GAP)
        elif pattern == "long_changing":
            starts |= set(GAP)
        starts.add(0)
    address = None
    for i in range(h):
        if i in starts:
            address = fresh(address)
        m[i][0] = address
    for i in (255, 256, 511):
        if i < h and pattern != "edges":
            m[i][1] = m[i][1] or PLUS    # not padding: the product absorbs them


def _memory_control(rng, m, pattern):
    h = len(m)
    dummy = [1] * h if pattern == "edges" else [rng.randrange(2) for _ in range(h)]
    if pattern == "gap":
        for i in GAP:
            dummy[i] = 1
    for i in EDGE_ROWS:
        if i < h and not (pattern == "gap" and i in GAP):
            dummy[i] = 0
    for i in range(h):
        m[i][3] = dummy[i]


def _linear(c1, c2, c3, x1, x2, x3):
    return xadd(xadd(xscale(c1, x1), xscale(c2, x2)), xscale(c3, x3))


def _group(index, spec):
    name, h, fill, ch, p_pat, i_pat, m_pat, in_len, out_len = spec
    rng = random.Random(0xE87E0000 + index)
    mode = "random" if ch == "random" else "palette"
    challenges = [_element(rng, mode) for _ in range(11)]
    if ch == "zero_evals":
        challenges[8] = challenges[9] = challenges[10] = X0
    initials = [_element(rng, mode) for _ in range(2)]
    matrices = {t: _fill(rng, fill, WIDTH[t], h, 3 * k + index) for k, t in enumerate(TABLES)}
    _processor_control(rng, matrices["processor"], p_pat)
    _instruction_control(rng, matrices["instruction"], fill, i_pat)
    _memory_control(rng, matrices["memory"], m_pat)
    for t, length in (("input", in_len), ("output", out_len)):
        for i in range(length, h):
            matrices[t][i][0] = 0        # padding rows of an IO table are zero rows
    zero_from = {}
    if name == "zero":
        a, b, c, d, e, f = challenges[:6]
        zp, zi, zm = ZERO_ROWS["processor"], ZERO_ROWS["instruction"], ZERO_ROWS["memory"]
        row = matrices["processor"][zp]
        row[2] = PLUS
        challenges[6] = _linear(a, b, c, row[1], row[2], row[3])          # alpha: the factor of this row is zero
        challenges[7] = _linear(d, e, f, row[0], row[4], row[5])          # beta
        matrices["instruction"][zi][:] = [row[1], row[2], row[3]]
        matrices["instruction"][zi - 1][0] = row[1]                       # the address repeats: a row of the product
        matrices["memory"][zm][:] = [row[0], row[4], row[5], 0]
        # the first row whose RECORDED value is zero: the processor and memory columns record the state before the row's update
        zero_from = {"processor": zp + 1, "instruction": zi, "memory": zm + 1}
    lengths = {"input": in_len, "output": out_len}
    cases = {}
    for t in TABLES:
        assert len(matrices[t]) == h and all(0 <= v < P for r in matrices[t] for v in r)
        cases[t] = {"name": "%s-%s" % (name, t), "group": name, "table": t, "height": h, "length": lengths.get(t, h), "matrix": matrices[t],
                    "challenges": challenges, "initials": initials, "zero_from": zero_from.get(t)}
    assert matrices["processor"][h - 1][2] != COMMA and matrices["instruction"][0][0] != P - 1
    return cases


_CACHE = {}


def groups():
    """-> list of {table: case}, one per entry of GROUPS"""
    if "groups" not in _CACHE:
        _CACHE["groups"] = [_group(k, spec) for k, spec in enumerate(GROUPS)]
    return _CACHE["groups"]


def cases(table):
    return [g[table] for g in groups()]


def row0_case():
    """instruction table of height 4 whose rows 0 and 1 have the address p - 1"""
    if "row0" not in _CACHE:
        rng = random.Random(0xE87E0FFF)
        matrix = [[P - 1, PLUS, OPEN], [P - 1, OPEN, DOT], [5, DOT, COMMA], [5, DOT, COMMA]]
        _CACHE["row0"] = {"name": "row0-instruction", "group": "row0", "table": "instruction", "height": 4, "length": 4, "matrix": matrix,
                          "challenges": [_element(rng, "random") for _ in range(11)], "initials": [_element(rng, "random") for _ in range(2)],
                          "zero_from": None}
    return _CACHE["row0"]


def all_cases():
    return [g[t] for g in groups() for t in TABLES] + [row0_case()]


def sample_rows(height):
    """the rows whose values the fixture keeps: 0, 1, 254 .. 257 and the last two"""
    return sorted({i for i in (0, 1, 254, 255, 256, 257, height - 2, height - 1) if 0 <= i < height})
