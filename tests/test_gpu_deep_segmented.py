"""BrainfuckStark.prove_deep(segmented=True) / verify_deep(segmented=True) on the MI355X ("Segmented composition"): the
decimation entry of include/bfstark_segments.h against numpy slicing, what it leaves alone (tests/painted.py), the stream it keeps to
(tests/deep_segments_stream_child.py) and its export; and the mode end to end: proof bytes equal to the committed fixtures, the committed
codewords against the CPU oracle's evaluation of the kept interpolants, the segments against the composition polynomial's coefficients, H
on its points against the weighted quotient sum in Python integers, the refusals, and the unsegmented mode untouched behind it.  Exact
integer arithmetic: every comparison is for equality.  Commitment domains here are 2^5 .. 2^11, working domains 2^6 .. 2^11."""
import ctypes
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import soundness_cases
from painted import Arena
from tools import deep_stark_time as deep
from tools import stark_fri_modes as modes
from tools.stark_fri_modes import mode

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
CHILD_SECONDS = 120
NAMES = list(deep.PROGRAMS)
FORTY = "+" * 40
P = soundness_cases.P
u64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def sb():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import stark_brainfuck_amd
    return stark_brainfuck_amd


_made = {}


def proved(name, m=None):
    """(stark, proof) of program `name` in the segmented mode on the seeded randomness with the intermediates kept, made once"""
    key = (name, json.dumps(m, sort_keys=True))
    if key not in _made:
        _made[key] = deep.prove_deep_seeded(name, m, prepare=lambda s: setattr(s, "keep_intermediates", True), segmented=True)
    return _made[key]


# ------------------------------------------------------------------------------------------------ 1. the decimation entry
@pytest.mark.parametrize("batch", [1, 3, 27])
@pytest.mark.parametrize("log_step", [0, 1, 2, 3, 4])
def test_decimate_rows_is_numpy_slicing(sb, oracle, batch, log_step):
    """n_out 1, 2, 63, 64, 65, 257 (below, at and above a wavefront; two blocks), dense and with stride_out > n_out, input rows with a
    tail behind the last word read; nothing outside the rows is written, the input is untouched"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer, current_stream, synchronize
    lib = _lib.load()
    for n_out in (1, 2, 63, 64, 65, 257):
        needed = ((n_out - 1) << log_step) + 1
        for stride_in, stride_out in ((needed, n_out), (needed + 5, n_out + 3)):
            source = oracle.felt_array(0x5E6 + n_out, 64 * log_step + batch, batch * stride_in)
            d_in = DeviceBuffer.from_numpy(source)
            arena = Arena(batch=batch, stride=stride_out, n=n_out)
            _lib.check(lib.bfsg_decimate_rows(d_in.ptr, stride_in, log_step, arena.ptr, stride_out, n_out, batch, current_stream()))
            synchronize()
            after = arena.contained(inputs=[("in", source, d_in.to_numpy())])
            want = source.reshape(batch, stride_in)[:, ::1 << log_step][:, :n_out]
            assert np.array_equal(arena.rows(after), want), (n_out, stride_in, stride_out)


def test_decimate_rows_refuses_bad_arguments_and_enqueues_nothing(sb):
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer, current_stream
    lib = _lib.load()
    d_in = DeviceBuffer.from_numpy(np.arange(4 * 64, dtype=np.uint64))
    arena = Arena(batch=4, stride=20, n=16)
    good = [d_in.ptr, 64, 2, arena.ptr, 20, 16, 4, current_stream()]

    def rc(at, value):
        return lib.bfsg_decimate_rows(*(good[:at] + [value] + good[at + 1:]))
    refused = {"no input": rc(0, None), "no output": rc(3, None), "log_step 33": rc(2, 33), "no words": rc(5, 0), "rows that overlap": rc(4, 15),
               "more words than 2^32": rc(5, (1 << 32) + 1), "more rows than a grid has": rc(6, 65536)}
    assert refused == {k: 6 for k in refused}
    assert b"bfsg_decimate_rows" in lib.bfs_last_error()
    assert rc(6, 0) == 0          # no rows: nothing to do, no error
    arena.contained()             # nothing was written


def test_decimate_rows_keeps_to_its_stream(sb):
    """tests/deep_segments_stream_child.py, once, in a child process under its own time limit"""
    proc = subprocess.run([sys.executable, os.path.join(HERE, "deep_segments_stream_child.py")], capture_output=True, text=True, timeout=CHILD_SECONDS)
    lines = [json.loads(l) for l in proc.stdout.splitlines() if l.startswith("{")]
    for l in lines:
        print(json.dumps(l))
    errors = [l["error"] for l in lines if "error" in l]
    assert proc.returncode == 0 and not errors and lines and lines[-1].get("done"), "the child ended with status %s: %s\n%s" % (
        proc.returncode, errors, proc.stderr[-2000:])
    assert [l["ok"] for l in lines if "control" in l] == [True]
    by_case = {l["case"]: l for l in lines if "case" in l}
    assert len(by_case) == 1
    for name, line in by_case.items():
        assert line["kind"] == "enqueues" and line["ok"], "%s: %s" % (name, "\n".join(line["failures"]))


def test_the_library_exports_what_the_segments_header_declares(sb):
    from stark_brainfuck_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "bfstark_segments.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bfsg_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("bfsg_")}
    assert declared == exported == set(_lib.segments_exported_symbols()) == {"bfsg_decimate_rows"}
    assert all(getattr(lib, name).argtypes for name in declared)
    taking = set(re.findall(r"\b(bfsg_[a-z0-9_]+)\s*\([^;]*void\*\s*stream\)", text))
    import deep_segments_stream_child as child
    assert taking == declared == {entry for case in child.segments_cases() for entry in case.entries}
    arguments = re.search(r"bfsg_decimate_rows\s*\(([^;]*)\)\s*;", text).group(1)
    assert len(arguments.split(",")) == len(_lib._SEGMENTS_SIGNATURES["bfsg_decimate_rows"][1]) == 8


# ------------------------------------------------------------------------------------------------ 2. end to end
CASES = [(name, mode()) for name in NAMES] + [("two_io", deep.MODE_A8C_G4)]
IDS = [deep.segmented_fixture_file(name, m)[len("deep_segmented_"):-len("_proof.bin")] for name, m in CASES]
LOOP_MODES = [m for name, m in modes.FIXTURES if name == "loop"]          # folded, coset leaves, ground


@pytest.mark.parametrize("name,m", CASES, ids=IDS)
def test_verify_deep_accepts_the_segmented_proof_and_the_bytes_are_the_fixtures(sb, name, m):
    stark, proof = proved(name, m)
    shape = stark.deep_segmented_shape()
    assert (shape.n, shape.w, shape.s) == (deep.SEGMENTED_DOMAINS[name], 2 * deep.SEGMENTED_DOMAINS[name], 8)
    assert (shape.fri.folding_factor, shape.fri.coset_leaves, shape.fri.grinding_bits) == (m["folding_factor"], m["coset_leaves"], m["grinding_bits"])
    assert deep.make_stark(name, m).verify_deep(proof, segmented=True) is True
    entry = next(e for e in deep.fixtures(listing=deep.SEGMENTED_FIXTURE_LIST) if e["file"] == deep.segmented_fixture_file(name, m))
    committed = open(os.path.join(GOLDEN, entry["file"]), "rb").read()
    assert hashlib.sha256(committed).hexdigest() == entry["proof_sha256"] and (entry["program"], entry["input"]) == deep.PROGRAMS[name]
    assert proof == committed
    assert sorted(stark.timing) == sorted(["pad", "base_lde", "base_commit", "extend", "ext_lde", "ext_commit", "composition", "composition_commit",
                                           "opening", "serialize"])


def test_every_segmented_fixture_is_proven_here():
    assert sorted(e["file"] for e in deep.fixtures(listing=deep.SEGMENTED_FIXTURE_LIST)) == sorted(deep.segmented_fixture_file(name, m) for name, m in CASES)


def test_forty_increments_in_the_default_mode(sb):
    stark, proof = proved(FORTY)
    shape = stark.deep_segmented_shape()
    assert (shape.L, shape.S, shape.s, shape.n, shape.w) == (256, 2048, 8, 1024, 2048)          # (one cell: a short memory trace, eight segments)
    assert deep.make_stark(FORTY).verify_deep(proof, segmented=True) is True
    assert len(stark._last["segments"]) == shape.s


def test_forty_instructions_with_four_segments(sb, oracle):
    """40 instructions whose memory trace has 142 rows (tests/test_deep_segmented_host.py): the memory table is the tallest, s = 4, and
    W = N' at expansion factor 4 -- the codewords are committed as they lie and H is computed on every point"""
    from test_deep_segmented_host import FOUR_SEGMENTS
    stark, proof = proved(FOUR_SEGMENTS)
    shape, last = stark.deep_segmented_shape(), stark._last
    assert (shape.L, shape.S, shape.s, shape.n, shape.w) == (512, 2048, 4, 2048, 2048)
    assert last["committed_base_codewords"] is last["working_base_codewords"] and last["committed_ext_codewords"] is last["working_ext_codewords"]
    assert deep.make_stark(FOUR_SEGMENTS).verify_deep(proof, segmented=True) is True
    assert deep.make_stark(FOUR_SEGMENTS).verify_deep(proof) is False
    assert len(last["segments"]) == 4 and last["plan"].widths == (16, 9, 4)
    _check_exactness(stark, oracle)


@pytest.mark.parametrize("m", LOOP_MODES, ids=[modes.mode_id(m) for m in LOOP_MODES])
def test_the_loop_in_the_folded_coset_leaf_and_ground_modes(sb, m):
    stark, proof = proved("loop", m)
    assert stark.deep_segmented_shape().n == 256
    assert deep.make_stark("loop", m).verify_deep(proof, segmented=True) is True
    assert deep.make_stark("loop").verify_deep(proof, segmented=True) is False          # not a proof of the default mode


def test_the_loop_at_expansion_factor_sixteen(sb, oracle):
    """W == N': the codewords are committed as they lie (no decimation), H is computed on every second point (log_step 1)"""
    m = mode(log_expansion_factor=4, security_level=4)
    stark, proof = proved("loop", m)
    shape, last = stark.deep_segmented_shape(), stark._last
    assert (shape.L, shape.S, shape.s, shape.n, shape.w) == (64, 512, 8, 1024, 1024) and shape.w // shape.S == 2
    assert last["committed_base_codewords"] is last["working_base_codewords"] and last["committed_ext_codewords"] is last["working_ext_codewords"]
    assert last["commitments"][0].codewords is last["working_base_codewords"]
    assert deep.make_stark("loop", m).verify_deep(proof, segmented=True) is True
    _check_exactness(stark, oracle)


def test_the_debug_switch_checks_degree_and_segments(sb, monkeypatch):
    """BFS_DEBUG=1: H on 2 S points interpolates to S coefficients for an honest trace (the same proof bytes) -- through a second
    extension of the kept interpolants at expansion factor 4, on the working domain at 16 -- and does not for a false one"""
    from stark_brainfuck_amd.vm import LazyTraceMatrix, VirtualMachine
    monkeypatch.setenv("BFS_DEBUG", "1")
    wide = mode(log_expansion_factor=4, security_level=4)
    assert deep.prove_deep_seeded("loop", segmented=True)[1] == proved("loop")[1]
    assert deep.prove_deep_seeded("loop", wide, segmented=True)[1] == proved("loop", wide)[1]
    with pytest.raises(AssertionError, match="composition polynomial has degree"):
        deep.prove_deep_seeded("loop", matrices=[_false_processor("loop")] + list(deep.claim("loop")[4])[1:], segmented=True)


# ------------------------------------------------------------------------------------------------ 3. exactness
def _planes(buffer, rows, n):
    return buffer.to_numpy()[:rows * n].reshape(rows, n)


def _rows_at(stark, base, ext, i):
    """per table its row of base and extension values (limb triples) at word i of the working codewords"""
    rows, b, x = [], 0, 0
    for t in stark.tables:
        bw, xw = t.base_width, t.full_width - t.base_width
        rows.append([(int(base[b + c, i]), 0, 0) for c in range(bw)] + [tuple(int(ext[x + 3 * c + l, i]) for l in range(3)) for c in range(xw)])
        b, x = b + bw, x + 3 * xw
    return rows


def _h_at(stark, x, cur, nxt):
    """the weighted quotient sum at the base-field point x from every table's row and next row: the verifier's left-hand side"""
    from stark_brainfuck_amd import air
    last = stark._last
    challenges, terminals = last["challenges"], [tuple(t) for t in last["terminals"]]
    weights = [tuple(int(v) for v in w) for w in last["weights"]]
    z = (x, 0, 0)
    boundary = air.xinv(air.xsub(z, air.X1))
    total, at, rows = air.X0, 0, []
    for t, c, n in zip(stark.tables, cur, nxt):
        if not t.height:
            rows.append([air.X0] * t.full_width)
            at += t.num_quotients()
            continue
        rows.append(c)
        off = air.xsub(z, (pow(t.omicron.value, P - 2, P), 0, 0))
        factors = {"boundary": boundary, "transition": air.xmul(off, air.xinv(air.xsub(air.xpow(z, t.height), air.X1))), "terminal": air.xinv(off)}
        params, memo = t.air_params(challenges), {}
        for kind, constraints in t.air.all():
            for e in constraints:
                value = air.evaluate(e, c, n, challenges, terminals, params, memo)
                total = air.xadd(total, air.xmul(air.xmul(weights[at], value), factors[kind]))
                at += 1
    for j, pa in enumerate(stark.permutation_arguments):
        total = air.xadd(total, air.xmul(air.xmul(weights[at + j], pa.evaluate_difference(rows)), boundary))
    assert at + 2 == len(weights)
    return total


def _check_exactness(stark, o):
    last, shape = stark._last, stark.deep_segmented_shape()
    L, S, s, n, w = shape.L, shape.S, shape.s, shape.n, shape.w
    assert (last["L"], last["S"], last["s"]) == (L, S, s)
    offset, omega_n, omega_w = shape.domain.offset.value, shape.domain.omega.value, shape.working_domain.omega.value
    # C0 and C1: the committed codewords are the kept interpolants on the n points, by the oracle
    base, ext = _planes(last["committed_base_codewords"], 16, n), _planes(last["committed_ext_codewords"], 27, n)
    for c, f in enumerate(last["base_polys"]):
        assert len(f) <= L and np.array_equal(base[c], o.fast_coset_evaluate(np.ascontiguousarray(f.to_numpy()), offset, omega_n, n)), "base column %d" % c
    for c, f in enumerate(last["ext_polys"]):
        for l, plane in enumerate(f.to_numpy()):
            assert np.array_equal(ext[3 * c + l], o.fast_coset_evaluate(np.ascontiguousarray(plane), offset, omega_n, n)), "extension column %d limb %d" % (c, l)
    assert last["commitments"][0].codewords is last["committed_base_codewords"] and last["commitments"][1].codewords is last["committed_ext_codewords"]
    assert [c.n for c in last["commitments"]] == [n, n, n]
    # ... and every (w / n)-th word of the working codewords
    wbase, wext = _planes(last["working_base_codewords"], 16, w), _planes(last["working_ext_codewords"], 27, w)
    assert np.array_equal(wbase[:, ::w // n], base) and np.array_equal(wext[:, ::w // n], ext)
    # C2: the segments tile the coefficients of H
    coefficients = last["h_coefficients"].to_numpy()
    assert coefficients.shape == (3, S) and len(last["segments"]) == s and all(len(f) == L for f in last["segments"])
    assert np.array_equal(np.concatenate([f.to_numpy() for f in last["segments"]], axis=1), coefficients)
    assert last["plan"].widths == (16, 9, s) and len(last["opened"][-1][0]) == s
    # H on its S points, every (w / S)-th of the working domain: the weighted quotient sum in Python integers, at the first and last point,
    # at points whose next row wraps around the end of the codewords, and at a few in between
    h_values = last["h_values"].to_numpy()
    assert h_values.shape == (3, S)
    step = w // S
    # the largest unit distance short of the whole domain (a table of one row is its own next row): points from S - distance / step on wrap
    distance = max(t.unit_distance(w) for t in stark.tables if t.unit_distance(w) < w)
    points = sorted({0, 1, S // 2, S // 3, S - 1, S - 2, S - distance // step, S - distance // step - 1, S - max(distance // step // 2, 1)})
    assert len(points) >= 8 and any((k * step + distance) >= w for k in points)
    for k in points:
        i = k * step
        cur = _rows_at(stark, wbase, wext, i)
        nxt = [_rows_at(stark, wbase, wext, (i + t.unit_distance(w)) % w)[j] for j, t in enumerate(stark.tables)]
        x = offset * pow(omega_w, i, P) % P
        assert tuple(int(v) for v in h_values[:, k]) == _h_at(stark, x, cur, nxt), "point %d" % k


@pytest.mark.parametrize("name", NAMES)
def test_the_commitments_the_segments_and_the_composition_are_exact(sb, oracle, name):
    stark, _ = proved(name)
    _check_exactness(stark, oracle)


# ------------------------------------------------------------------------------------------------ 4. refusals, and the other mode untouched
def _false_processor(name):
    from stark_brainfuck_amd.vm import LazyTraceMatrix, VirtualMachine
    values = np.array(deep.claim(name)[4][0].values, dtype=np.uint64)
    values[1, 5] = (int(values[1, 5]) + 1) % P          # the memory value of the second cycle
    return LazyTraceMatrix(np.ascontiguousarray(values), VirtualMachine.field)


def _refused(stark, proof, capsys, **kwargs):
    capsys.readouterr()
    verdict = stark.verify_deep(proof, **kwargs)
    printed = capsys.readouterr().out
    assert printed.count("\n") == 1, "a refusal prints one line: %r" % printed
    return verdict


@pytest.mark.parametrize("name", ["io", "loop"])
def test_false_traces_and_tampered_segmented_proofs_are_refused(sb, name, capsys):
    stark, proof = proved(name)
    verifier = deep.make_stark(name)
    assert verifier.verify_deep(proof, segmented=True) is True
    false_proof = deep.prove_deep_seeded(name, matrices=[_false_processor(name)] + list(deep.claim(name)[4])[1:], segmented=True)[1]
    assert isinstance(false_proof, bytes) and false_proof != proof
    verdicts = {"a false trace": _refused(verifier, false_proof, capsys, segmented=True)}
    flipped = bytearray(proof)
    flipped[len(flipped) // 3] ^= 0x10
    verdicts["a flipped byte"] = _refused(verifier, bytes(flipped), capsys, segmented=True)
    changed = dict(deep.tamperings(proof))
    changed.update(deep.segment_tamperings(proof))
    for what, data in changed.items():
        verdicts[what] = _refused(verifier, data, capsys, segmented=True)
    verdicts["given to the unsegmented verifier"] = _refused(verifier, proof, capsys)
    verdicts["an unsegmented proof"] = _refused(verifier, deep.prove_deep_seeded(name)[1], capsys, segmented=True)
    assert verdicts == {what: False for what in verdicts} and len(verdicts) == 10
    assert verifier.verify_deep(proof, segmented=True) is True


def test_an_unsegmented_proof_after_a_segmented_one_is_the_fixture(sb):
    """one object, one process: the second Fri and the working-domain codewords of a segmented proof leave nothing behind"""
    from stark_brainfuck_amd import randomness
    stark = deep.make_stark("plus1")
    program, matrices = deep.claim("plus1")[0], deep.claim("plus1")[4]
    with randomness.override(modes.Stream(deep.seed_tag("plus1"))):
        segmented = stark.prove_deep(program, *matrices, segmented=True)
    with randomness.override(modes.Stream(deep.seed_tag("plus1"))):
        plain = stark.prove_deep(program, *matrices)
    assert plain == open(os.path.join(GOLDEN, "deep_plus1_proof.bin"), "rb").read()
    assert segmented == open(os.path.join(GOLDEN, "deep_segmented_plus1_proof.bin"), "rb").read()
    assert stark.fri.domain.length == deep.DOMAINS["plus1"] and stark.verify_deep(plain) is True and stark.verify_deep(segmented, segmented=True) is True
