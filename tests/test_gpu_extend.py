"""The extension stage on the device against models on plain integers, exactly, word for word.

  bfs_xfe_scan_device, bfs_xfe_scan_device_many   against scan_model.scan (the primitive as include/bfstark.h defines it), NOT against
                                                  the host primitive: at every edge of the partition of scan_fill (csrc/scan.hip)
  lde_tables + extend_tables_device               against extend_model (the reference's loops, pinned on the reference's own output in
                                                  golden/extend.json by test_extend_host.py) on the synthetic tables of extend_cases.py
  bfs_trace_pad                                   its scan masks on the same tables against the masks of the scan form

The native stage driver's scan list (the `add(...)` list of csrc/prover.cpp) cannot be fed synthetic tables: it takes a program, not a
table.  It stays covered by the tests that compare the proofs of both drivers byte for byte (test_gpu_stark.py), whose Python side is
the `_scans` lists pinned here, and its masks are the ones bfs_trace_pad writes."""
import ctypes

import numpy as np
import pytest

import extend_cases
import scan_cases
import scan_model
from extend_harness import ALL_CASES, expected, make_table, planes, scan_statement, table_terminals

P = scan_model.P
u64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from stark_brainfuck_amd import _lib
    return _lib.load()            # raises BackendUnavailable if the HIP library is missing: no fallback


class Uploads:
    """the operand columns and masks of the configurations of one test in HBM, each uploaded once"""

    def __init__(self, lib):
        from stark_brainfuck_amd.device import current_stream
        self.lib, self.stream, self.held = lib, current_stream(), {}

    def columns(self, n, mode):
        from stark_brainfuck_amd.device import DeviceBuffer
        key = ("columns", n, mode)
        if key not in self.held:
            self.held[key] = DeviceBuffer.from_numpy(np.array(scan_cases.operands(n, mode)[0], dtype=np.uint64).reshape(-1))
        return self.held[key]

    def mask(self, n, name):
        from stark_brainfuck_amd import _lib
        from stark_brainfuck_amd.device import DeviceBuffer
        key = ("mask", n, name)
        if key not in self.held:
            m8 = np.array(scan_cases.mask(n, name), dtype=np.uint8)
            buf = DeviceBuffer((n + 7) // 8)
            _lib.check(self.lib.bfs_memcpy_h2d(buf.ptr, m8.ctypes.data, n, self.stream))
            self.held[key] = (buf, m8)
        return self.held[key][0]

    def arguments(self, cfg):
        """-> (x1, x2, x3, mask pointers, constants, initial) of a configuration"""
        n = cfg["n"]
        d_cols = self.columns(n, cfg["mode"])
        ptrs = [d_cols.ptr + 8 * c * n if present else None for c, present in enumerate(cfg["present"])]
        d_mask = self.mask(n, cfg["mask_name"]).ptr if cfg["mask"] is not None else None
        flat = [v for c in cfg["constants"] for v in c]
        return ptrs, d_mask, (u64 * 12)(*flat), (u64 * 3)(*cfg["initial"])


def model(cfg):
    want, terminal = scan_model.scan(cfg["kind"], cfg["columns"], cfg["mask"], cfg["n"], cfg["constants"], cfg["initial"], cfg["before"], cfg["shift1"])
    return np.array(want, dtype=np.uint64), terminal


def check_against_model(cfg, got, terminals):
    want, want_terminal = model(cfg)
    assert (got < np.uint64(P)).all(), cfg["label"]
    assert np.array_equal(got, want), (cfg["label"], np.argwhere(got != want)[:4].tolist())
    for terminal in terminals:
        assert all(v < P for v in terminal) and tuple(terminal) == want_terminal, cfg["label"]
    if cfg["mask_name"] == "none":            # no row takes part: the initial value everywhere, and as the terminal
        assert want_terminal == tuple(cfg["initial"]) and all((plane == v).all() for plane, v in zip(got, cfg["initial"]))
    if cfg["zero_row"] is not None:
        first = cfg["zero_row"] + (1 if cfg["before"] else 0)
        assert want_terminal == (0, 0, 0) and not got[:, first:].any()
        # (palette cells repeat every 15 rows, and the zero factor with them: only random cells keep every earlier state non-zero)
        assert cfg["mode"] == "palette" or got[:, :first].any(axis=0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", scan_cases.SMALL_SIZES + scan_cases.LARGE_SIZES)
def test_device_scan_matches_the_model(lib, n):
    """bfs_xfe_scan_device against scan_model, one scan per call.  1, 255, 256, 257 rows: both kinds x every set of present columns (none
    included) x masks (absent, all zero, only row 0, only row n - 1, zero across whole workgroups) x recording before / after, on palette
    and random operands; shift1 in {0, 1, n - 1, n, n + 1} on a first column of distinct values; c0 = 0; a factor that is exactly zero
    in the middle and at the edges of a workgroup.  65 535 .. 131 073 rows (rows per thread 1 -> 2 -> 3, a last workgroup of one row): a
    handful of configurations each.  Every output word and both terminals (device and host copy)."""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer
    up = Uploads(lib)
    out, d_terminal = DeviceBuffer(3 * n), DeviceBuffer(3)
    configs = scan_cases.small_configs(n) if n in scan_cases.SMALL_SIZES else scan_cases.large_configs(n)
    for cfg in configs:
        ptrs, d_mask, constants, initial = up.arguments(cfg)
        terminal = (u64 * 3)()
        _lib.check(lib.bfs_xfe_scan_device(cfg["kind"], ptrs[0], ptrs[1], ptrs[2], cfg["shift1"], d_mask, n, constants, initial,
                                           1 if cfg["before"] else 0, out.ptr, n, d_terminal.ptr, terminal, up.stream))
        check_against_model(cfg, out.to_numpy(3 * n).reshape(3, n), [tuple(int(v) for v in terminal), tuple(int(v) for v in d_terminal.to_numpy(3))])


@pytest.mark.gpu
def test_scans_side_by_side_match_the_model(lib):
    """ONE call of bfs_xfe_scan_device_many with 64 scans, the most it takes: kinds, sizes 1 .. 1000 and two large ones (65 537 and
    131 073 rows, so that the launch is 256 workgroups wide and most scans leave most of it idle), masks, shifts and recording modes
    mixed; every scan against scan_model"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer
    up = Uploads(lib)
    configs = scan_cases.many_configs()
    assert len(configs) == 64 and {c["kind"] for c in configs} == {0, 1} and {c["before"] for c in configs} == {True, False}
    specs, outs = [], []
    for cfg in configs:
        n = cfg["n"]
        ptrs, d_mask, constants, initial = up.arguments(cfg)
        out, d_terminal = DeviceBuffer(3 * n), DeviceBuffer(3)
        specs.append(_lib.ScanSpec(cfg["kind"], 1 if cfg["before"] else 0, ptrs[0], ptrs[1], ptrs[2], cfg["shift1"], d_mask, n, constants, initial,
                                   out.ptr, n, d_terminal.ptr))
        outs.append((out, d_terminal))
    _lib.check(lib.bfs_xfe_scan_device_many((_lib.ScanSpec * 64)(*specs), 64, up.stream))
    for cfg, (out, d_terminal) in zip(configs, outs):
        check_against_model(cfg, out.to_numpy(3 * cfg["n"]).reshape(3, cfg["n"]), [tuple(int(v) for v in d_terminal.to_numpy(3))])


# ---- the tables
def domain_2_11():
    from stark_brainfuck_amd.algebra import BaseField
    from stark_brainfuck_amd.fri import Fri
    field = BaseField.main()
    return Fri.Domain(field.generator(), field.primitive_nth_root(1 << 11), 1 << 11)


def extend_on_the_device(cases):
    """lde_tables on a 2^11 domain, then extend_tables_device, for the tables of `cases` (same challenges and initials) in one call each;
    compares _ext_device and the terminals with the model"""
    from stark_brainfuck_amd.table import extend_tables_device, lde_tables
    tables = [make_table(c) for c in cases]
    lde_tables(tables, domain_2_11())
    extend_tables_device(tables, cases[0]["challenges"], cases[0]["initials"])
    for case, t in zip(cases, tables):
        assert case["challenges"] is cases[0]["challenges"] or case["challenges"] == cases[0]["challenges"]
        columns, terminals = expected(case["name"])
        h, w = case["height"], len(columns)
        got = t._ext_device.to_numpy(3 * w * h).reshape(w, 3, h)
        assert t.ext_columns is None and (got < np.uint64(P)).all(), case["name"]
        for k, col in enumerate(columns):
            assert np.array_equal(got[k], planes(col)), (case["name"], k, np.argwhere(got[k] != planes(col))[:4].tolist())
        assert [tuple(int(v) for v in x) for x in table_terminals(t, case["table"])] == terminals, case["name"]


@pytest.mark.gpu
@pytest.mark.parametrize("group", [g[0] for g in extend_cases.GROUPS])
def test_five_tables_extended_in_one_call_match_the_model(lib, group):
    """extend_tables_device on the five tables of a group of extend_cases.py together (nine scans in one launch): every word of every
    extension column in HBM and every terminal against extend_model"""
    g = extend_cases.groups()[[s[0] for s in extend_cases.GROUPS].index(group)]
    extend_on_the_device([g[t] for t in extend_cases.TABLES])


@pytest.mark.gpu
@pytest.mark.parametrize("table", extend_cases.TABLES)
def test_each_table_extended_on_its_own_matches_the_model(lib, table):
    """the same with one call per table (Table.lde, Table.extend_device's path), for every case of the table -- the instruction table's
    list ends with the table whose first address is p - 1, which keeps row 0 out of the running evaluation"""
    cases = [c for c in ALL_CASES.values() if c["table"] == table]
    assert len(cases) == len(extend_cases.GROUPS) + (table == "instruction")
    for case in cases:
        extend_on_the_device([case])


@pytest.mark.gpu
def test_padding_writes_the_masks_of_the_scan_form(lib):
    """bfs_trace_pad on the synthetic tables, given whole (rows = height: nothing to append) and, for the row-0 table, one row short:
    the padded columns are the table, and the masks are the ones the scan form (extend_harness.scan_statement, held equal to
    extend_model by test_extend_host.py) uses -- these are the masks the native stage driver's scans run with"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer
    kinds = {t: k for k, t in enumerate(extend_cases.TABLES)}
    row0 = extend_cases.row0_case()
    short = dict(row0, matrix=row0["matrix"][:3] + [[row0["matrix"][2][0], 0, 0]])          # what padding makes of the first three rows
    jobs = [[g[t] for t in extend_cases.TABLES] for g in extend_cases.groups()] + [[row0], [short]]
    for cases in jobs:
        structs, held = (_lib.TracePadTable * len(cases))(), []
        for s, case in zip(structs, cases):
            h, w = case["height"], extend_cases.WIDTH[case["table"]]
            given = case["matrix"][:3] if case is short else case["matrix"]
            raw = DeviceBuffer.from_numpy(np.array(given, dtype=np.uint64).reshape(-1))
            out, masks = DeviceBuffer(w * h), [DeviceBuffer((h + 7) // 8) for _ in range(3)]
            held.append((raw, out, masks))
            s.d_rows, s.rows, s.row_stride, s.height = raw.ptr, len(given), w, h
            s.d_out, s.d_mask0, s.d_mask1, s.d_mask2, s.kind, s.width = out.ptr, masks[0].ptr, masks[1].ptr, masks[2].ptr, kinds[case["table"]], w
        _lib.check(lib.bfs_trace_pad(structs, len(cases), 0))
        for case, (raw, out, masks) in zip(cases, held):
            h, w = case["height"], extend_cases.WIDTH[case["table"]]
            assert out.to_numpy(w * h).reshape(w, h).T.tolist() == case["matrix"], case["name"]
            statement = scan_statement(case)
            which = {"processor": (0, 2, 3), "instruction": (0, 1), "memory": (0,)}.get(case["table"], ())      # IO tables: no masks
            want = [statement[k][2] for k in which]
            for k, mask in enumerate(want):
                got = masks[k].to_numpy((h + 7) // 8).view(np.uint8)[:h]
                assert got.tolist() == [int(v) for v in mask], (case["name"], k)
    assert scan_statement(row0)[1][2][0] is False and scan_statement(extend_cases.cases("instruction")[0])[1][2][0] is True
