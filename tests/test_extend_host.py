"""The extension stage on the host, exactly, word for word (no GPU needed).

  reference  --extend.json-->  extend_model  -->  Table.extend of the five table classes (`_scans`, `_make_scan_masks`, bfs_xfe_scan)
                               scan_model    -->  Table.scan (the host primitive bfs_xfe_scan)

tests/golden/extend.json holds what the reference's own `extend` made of the synthetic tables of extend_cases.py (full-range cells,
products that meet a zero factor, mask patterns no program produces); extend_model.py restates the reference's loops on integers and must
reproduce every digest, sample and terminal of it; the package must then equal the model in every word.  tests/test_gpu_extend.py holds
the device against the same two models."""
import hashlib
import struct

import numpy as np
import pytest

import extend_cases
import scan_cases
import scan_model
from conftest import load_golden
from extend_harness import ALL_CASES, expected, make_table, planes, scan_statement, table_terminals

P = scan_model.P


@pytest.fixture(scope="session")
def sb():
    from stark_brainfuck_amd import build
    build.build_library()
    import stark_brainfuck_amd
    return stark_brainfuck_amd


def test_the_case_lists_hold_what_they_promise():
    """every table has a case per group, heights 512, 1 and 2; every branch of the loops occurs; the planted zero factor empties every
    later state; the row-0 case starts with the address p - 1"""
    for table in extend_cases.TABLES:
        cases = extend_cases.cases(table)
        assert sorted({c["height"] for c in cases}) == [1, 2, 512] and len(cases) == len(extend_cases.GROUPS)
        assert all(0 <= v < P for c in cases for row in c["matrix"] for v in row)
    big = [g for g in extend_cases.groups() if g["processor"]["height"] == 512]
    ci = {v for g in big for row in g["processor"]["matrix"] for v in [row[2]]}
    assert {0, ord(","), ord("."), ord("+"), P - 1} <= ci
    assert all(g["processor"]["matrix"][-1][2] != ord(",") for g in extend_cases.groups())
    for what, mask_of in (("active", lambda row: row[2] != 0), ("reads", lambda row: row[2] == ord(",")), ("writes", lambda row: row[2] == ord("."))):
        masks = [[mask_of(row) for row in g["processor"]["matrix"]] for g in big]
        for edge in extend_cases.EDGE_ROWS:
            assert any(m[edge] for m in masks) or (edge == 511 and what == "reads"), (what, edge)       # (',' cannot stand on the last row)
        assert any(not any(m[120:401]) for m in masks)                                     # more than 256 rows in a row left out
    same = [[i > 0 and m[i][0] == m[i - 1][0] for i in range(512)] for m in (g["instruction"]["matrix"] for g in big)]
    product = [[s and row[1] != 0 for s, row in zip(ss, g["instruction"]["matrix"])] for ss, g in zip(same, big)]
    assert any(all(p[i] for i in (255, 256, 511)) for p in product) and any(not any(p[120:401]) for p in product)
    assert any(all(not s[i] for i in (255, 256, 511)) for s in same) and any(all(s[120:401]) for s in same)
    assert any(row[1] == 0 for g in big for row in g["instruction"]["matrix"])
    dummies = [[row[3] for row in g["memory"]["matrix"]] for g in big]
    assert {v for d in dummies for v in d} == {0, 1} and any(all(d[120:401]) for d in dummies)
    assert all(any(d[i] == 0 for d in dummies) for i in extend_cases.EDGE_ROWS)
    assert any(g["processor"]["challenges"][8] == g["processor"]["challenges"][9] == g["processor"]["challenges"][10] == (0, 0, 0) for g in big)
    for table in ("processor", "instruction", "memory"):
        case = next(c for c in extend_cases.cases(table) if c["zero_from"] is not None)
        columns, terminals = expected(case["name"])
        for k in ((0, 1) if table == "processor" else (0,)):
            col = columns[k]
            assert all(any(v) for v in col[:case["zero_from"]]) and not any(any(v) for v in col[case["zero_from"]:]) and terminals[k] == (0, 0, 0)
    row0 = extend_cases.row0_case()
    assert row0["matrix"][0][0] == P - 1 and all(g["instruction"]["matrix"][0][0] != P - 1 for g in extend_cases.groups())


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_model_reproduces_the_reference(name):
    """extend_model against what the reference's extend made of the same table (golden/gen_extend_golden.py): the SHA-256 of every
    extension column, its values at rows 0, 1, 254 .. 257 and the last two, and every terminal"""
    golden = load_golden("extend.json")
    assert set(golden) == set(ALL_CASES)
    want, case = golden[name], ALL_CASES[name]
    columns, terminals = expected(name)
    assert want["height"] == case["height"] and len(columns) == len(want["columns"]) == extend_cases.EXT_WIDTH[case["table"]]
    for col, rec in zip(columns, want["columns"]):
        assert len(col) == case["height"] and all(0 <= v < P for t in col for v in t)
        assert hashlib.sha256(b"".join(struct.pack("<3Q", *v) for v in col)).hexdigest() == rec["sha256"]
        assert [s[0] for s in rec["samples"]] == extend_cases.sample_rows(case["height"])
        assert [[i] + list(col[i]) for i in extend_cases.sample_rows(case["height"])] == rec["samples"]
    assert [list(t) for t in terminals] == want["terminals"]


def test_the_reference_leaves_row_zero_out_when_its_address_is_minus_one():
    """instruction_table.py:184 starts `previous_address` at -1: the fixture's evaluation column of the row-0 case is zero on rows 0 and
    1 (both addresses are p - 1) and absorbs row 2"""
    rec = load_golden("extend.json")["row0-instruction"]["columns"][1]["samples"]
    assert rec[0] == [0, 0, 0, 0] and rec[1] == [1, 0, 0, 0] and any(rec[2][1:])


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_table_extend_matches_the_model(sb, name):
    """Table.extend of the package's table classes -- the scans of `_scans` with the masks of `_make_scan_masks`, run by the host
    primitive -- against extend_model: every word of every extension column, every terminal"""
    case = ALL_CASES[name]
    t = make_table(case)
    t.extend(case["challenges"], case["initials"])
    columns, terminals = expected(name)
    assert len(t.ext_columns) == len(columns)
    for k, col in enumerate(columns):
        got = t.ext_columns[k]
        assert got.shape == (3, case["height"]) and (got < np.uint64(P)).all()
        assert np.array_equal(got, planes(col)), (name, k)
    assert [tuple(int(v) for v in x) for x in table_terminals(t, case["table"])] == terminals


def run_host_scan(cfg):
    from stark_brainfuck_amd.table import Table
    n = cfg["n"]
    cols = [np.array(c, dtype=np.uint64) if c is not None else None for c in cfg["columns"]]
    if cols[0] is not None and cfg["shift1"] % n:
        cols[0] = np.roll(cols[0], -(cfg["shift1"] % n))          # the host primitive has no shift: Table.extend rolls the column too
    mask = np.array(cfg["mask"], dtype=bool) if cfg["mask"] is not None else None
    if all(c is None for c in cols) and mask is None:
        mask = np.ones(n, dtype=bool)                             # (Table.scan takes the row count from its arrays)
    return Table.scan(cfg["kind"], cols, mask, cfg["constants"], cfg["initial"], cfg["before"])


@pytest.mark.parametrize("n", scan_cases.SMALL_SIZES)
def test_host_scan_matches_the_model(sb, n):
    """Table.scan (bfs_xfe_scan, csrc/hostscan.cpp) against scan_model on the configurations the device is tested with: both kinds,
    every set of present columns, every mask, both recording modes, palette and random operands, shifts, c0 = 0, planted zero factors"""
    for cfg in scan_cases.small_configs(n):
        want, want_terminal = scan_model.scan(cfg["kind"], cfg["columns"], cfg["mask"], n, cfg["constants"], cfg["initial"], cfg["before"], cfg["shift1"])
        got, terminal = run_host_scan(cfg)
        assert (got < np.uint64(P)).all() and np.array_equal(got, np.array(want, dtype=np.uint64)), cfg["label"]
        assert terminal == want_terminal, cfg["label"]
        if cfg["mask_name"] == "none":
            assert terminal == tuple(cfg["initial"]) and all(set(p) == {v} for p, v in zip(want, cfg["initial"]))
        if cfg["zero_row"] is not None:
            assert terminal == (0, 0, 0)


# ---- the guard: the cases tell neighbouring rules apart
def run_statement(s, n):
    kind, cols, mask, constants, initial, before, shift1 = s
    out, _ = scan_model.scan(kind, cols, mask, n, constants, initial, before, shift1)
    return list(zip(*out))


def test_the_cases_tell_neighbouring_rules_apart():
    """for every case and extension column: the scan form gives the model's column, and recording the state on the other side of the
    update, reading the first column one row further (or not), and inverting the mask each give ANOTHER column at height 512 (heights 1
    and 2 have too few rows to differ in every rule).  So a scan list, mask or primitive that slips to a neighbouring rule cannot pass test_table_extend_matches_the_model."""
    for name, case in ALL_CASES.items():
        n = case["height"]
        columns, _ = expected(name)
        for k, s in enumerate(scan_statement(case)):
            kind, cols, mask, constants, initial, before, shift1 = s
            assert run_statement(s, n) == columns[k], (name, k)
            if n < 512:
                continue
            inverted = [0] * n if mask is None else [not v for v in mask]
            neighbours = {"before": (kind, cols, mask, constants, initial, not before, shift1),
                          "shift": (kind, cols, mask, constants, initial, before, 1 - shift1),
                          "mask": (kind, cols, inverted, constants, initial, before, shift1)}
            for rule, other in neighbours.items():
                # (a first column that holds one value everywhere -- the "constant" group -- reads the same a row further)
                same_allowed = rule == "shift" and len(set(cols[0])) == 1
                assert (run_statement(other, n) == columns[k]) == same_allowed, (name, k, rule)
