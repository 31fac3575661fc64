"""BrainfuckStark.prove_deep / verify_deep on the MI355X ("Proving by out-of-domain openings"): the composition kernels of
include/bfstark_compose.h against the written-out quotients, what they leave alone (tests/painted.py), the stream they keep to
(tests/deep_compose_stream_child.py) and their exports; PolynomialCommitment.commit_evaluated against commit; and the mode end to end:
proof bytes equal to the committed fixtures, the opened values recomputed from the coefficients, the verifier's identity through the
MPolynomial presentation of the constraints, and the refusals.  Exact integer arithmetic: every comparison is for equality.

Four programs reach every shape of the opening plan: "+" (2^8, both I/O tables empty), ",." (2^9, I/O tables of height 1), ",.,." (2^10,
height 2) and "++[>+<-]>." (2^11, input empty, output of height 1)."""
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

from painted import Arena
from tools import deep_stark_time as deep
from tools.stark_fri_modes import mode

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
CHILD_SECONDS = 120
NAMES = list(deep.PROGRAMS)
u64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def sb():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import stark_brainfuck_amd
    return stark_brainfuck_amd


_made = {}


def proved(name, m=None):
    """(stark, proof) of program `name` on the seeded randomness with the intermediates kept, made once"""
    key = (name, json.dumps(m, sort_keys=True))
    if key not in _made:
        _made[key] = deep.prove_deep_seeded(name, m, prepare=lambda s: setattr(s, "keep_intermediates", True))
    return _made[key]


def _xfe():
    from stark_brainfuck_amd import air
    return air


# ------------------------------------------------------------------------------------------------ 1. the composition kernels
def _written_out(stark):
    """sum beta * q over Table.all_quotients and PermutationArgument.quotient, read back and summed in Python integers -> (3, n) objects"""
    air = _xfe()
    last, domain, n = stark._last, stark.fri.domain, stark.fri.domain.length
    weights = [tuple(int(v) for v in w) for w in last["weights"]]
    total, at = (np.zeros(n, dtype=object),) * 3, 0
    for t in stark.tables:
        nq = t.num_quotients()
        if t.height:
            q = t.all_quotients(domain, None, last["challenges"], last["terminals"]).to_numpy().reshape(nq, 3, n).astype(object)
            for k in range(nq):
                total = air.xadd(total, air.xmul(weights[at + k], tuple(q[k])))
        at += nq
    for j, pa in enumerate(stark.permutation_arguments):
        q = pa.quotient(domain).to_numpy().reshape(3, n).astype(object)
        total = air.xadd(total, air.xmul(weights[at + j], tuple(q)))
    return np.stack(total)


def _compose_calls(stark, log_step, out_ptr):
    """the calls of BrainfuckStark.compose_into, one by one: functions of the accumulate flag"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import current_stream
    from stark_brainfuck_amd.table import _air_arguments
    lib, last, domain, n = _lib.load(), stark._last, stark.fri.domain, stark.fri.domain.length
    weights, calls, at = np.ascontiguousarray(last["weights"], dtype=np.uint64), [], 0
    limbs = lambda w: np.ascontiguousarray(w).reshape(-1).ctypes.data_as(ctypes.POINTER(u64))
    for t in stark.tables:
        nq = t.num_quotients()
        if t.height:
            calls.append(lambda accumulate, t=t, w=weights[at:at + nq].copy(): _lib.check(lib.bfsc_air_compose(
                t.table_index, t.base_codewords.ptr, t.ext_codewords.ptr, *t._domain_arguments(domain), *_air_arguments(t, last["challenges"], last["terminals"]),
                limbs(w), log_step, accumulate, out_ptr, current_stream())))
        at += nq
    for j, pa in enumerate(stark.permutation_arguments):
        lt, rt = stark.tables[pa.lhs[0]], stark.tables[pa.rhs[0]]
        calls.append(lambda accumulate, lt=lt, rt=rt, pa=pa, w=weights[at + j].copy(): _lib.check(lib.bfsc_difference_compose(
            lt.ext_codeword_ptr(pa.lhs[1]), rt.ext_codeword_ptr(pa.rhs[1]), n.bit_length() - 1, domain.offset.value, domain.omega.value, limbs(w),
            log_step, accumulate, out_ptr, current_stream())))
    return calls


_sums = {}


@pytest.mark.parametrize("log_step", [0, 2])
@pytest.mark.parametrize("name", NAMES)
def test_the_composition_is_the_weighted_sum_of_the_written_out_quotients(sb, name, log_step):
    """into a painted buffer, the first call with accumulate = 0, in table order and in reversed order; every point for step 1, every
    fourth point of the same sum for step 4; nothing beyond the 3 * (n >> log_step) words is written"""
    stark, _ = proved(name)
    n = stark.fri.domain.length
    assert n == deep.DOMAINS[name] and (stark.input_table.height, stark.output_table.height) == deep.HEIGHTS[name]
    if name not in _sums:
        _sums[name] = _written_out(stark)
    want = np.array([[int(v) for v in plane[::1 << log_step]] for plane in _sums[name]], dtype=np.uint64)
    count = n >> log_step
    for order in (1, -1):
        arena = Arena(batch=3, stride=count, n=count)
        calls = _compose_calls(stark, log_step, arena.ptr)[::order]
        assert len(calls) == sum(1 for t in stark.tables if t.height) + 2
        for k, call in enumerate(calls):
            call(0 if k == 0 else 1)
        got = arena.rows(arena.contained())
        assert np.array_equal(got, want), "order %d" % order
    # the prover's own H on the d points is this sum on every expansion_factor-th point
    if log_step == 2:
        assert stark.expansion_factor == 4 and np.array_equal(stark._last["h_values"].to_numpy(), want)


def test_the_entries_refuse_bad_arguments_and_enqueue_nothing(sb):
    from stark_brainfuck_amd import _lib
    stark, _ = proved("plus1")
    lib = _lib.load()
    n = stark.fri.domain.length
    arena = Arena(batch=3, stride=n, n=n)
    t = stark.processor_table
    from stark_brainfuck_amd.table import _air_arguments
    ch, tm, pr = _air_arguments(t, stark._last["challenges"], stark._last["terminals"])
    w = (u64 * (3 * t.num_quotients()))()
    log_n, ud, h, oinv, offset, omega = t._domain_arguments(stark.fri.domain)
    good = [0, t.base_codewords.ptr, t.ext_codewords.ptr, log_n, ud, h, oinv, offset, omega, ch, tm, pr, w, 0, 0, arena.ptr, None]

    def rc(**change):
        args = list(good)
        for at, value in change.items():
            args[int(at[1:])] = value
        return lib.bfsc_air_compose(*args)
    refused = {"table 5": rc(a0=5), "table -1": rc(a0=-1), "log_step past log_n": rc(a13=log_n + 1), "log_n 33": rc(a3=33), "no base": rc(a1=None),
               "no ext": rc(a2=None), "no accumulator": rc(a15=None), "no challenges": rc(a9=None), "no terminals": rc(a10=None), "no weights": rc(a12=None)}
    assert refused == {k: 6 for k in refused}
    assert rc(a5=3) == 1          # BFS_ERR_NOT_POW2
    d = [t.ext_codewords.ptr, t.ext_codewords.ptr, log_n, offset, omega, (u64 * 3)(1, 2, 3), 0, 0, arena.ptr, None]
    assert [lib.bfsc_difference_compose(*(d[:k] + [v] + d[k + 1:])) for k, v in ((0, None), (1, None), (5, None), (8, None), (6, log_n + 1), (2, 33))] == [6] * 6
    arena.contained()             # nothing was written


def test_both_entries_keep_to_their_stream(sb):
    """tests/deep_compose_stream_child.py, once, in a child process under its own time limit"""
    proc = subprocess.run([sys.executable, os.path.join(HERE, "deep_compose_stream_child.py")], capture_output=True, text=True, timeout=CHILD_SECONDS)
    lines = [json.loads(l) for l in proc.stdout.splitlines() if l.startswith("{")]
    for l in lines:
        print(json.dumps(l))
    errors = [l["error"] for l in lines if "error" in l]
    assert proc.returncode == 0 and not errors and lines and lines[-1].get("done"), "the child ended with status %s: %s\n%s" % (
        proc.returncode, errors, proc.stderr[-2000:])
    assert [l["ok"] for l in lines if "control" in l] == [True]
    by_case = {l["case"]: l for l in lines if "case" in l}
    assert len(by_case) == 2
    for name, line in by_case.items():
        assert line["kind"] == "enqueues" and line["ok"], "%s: %s" % (name, "\n".join(line["failures"]))


def test_the_library_exports_what_the_header_declares(sb):
    from stark_brainfuck_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "bfstark_compose.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bfsc_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("bfsc_")}
    assert declared == exported == set(_lib.compose_exported_symbols()) == {"bfsc_air_compose", "bfsc_difference_compose"}
    assert all(getattr(lib, name).argtypes for name in declared)
    # every stream-taking function of the header is a case of the child above
    taking = set(re.findall(r"\b(bfsc_[a-z0-9_]+)\s*\([^;]*void\*\s*stream\)", text))
    import deep_compose_stream_child as child
    assert taking == declared == {entry for case in child.compose_cases() for entry in case.entries}
    # the signature table has the header's argument counts
    for name, count in (("bfsc_air_compose", 17), ("bfsc_difference_compose", 10)):
        arguments = re.search(name + r"\s*\(([^;]*)\)\s*;", text).group(1)
        assert len(arguments.split(",")) == len(_lib._COMPOSE_SIGNATURES[name][1]) == count


# ------------------------------------------------------------------------------------------------ 2. commit_evaluated
@pytest.mark.parametrize("kind", ["extension", "base"])
def test_commit_evaluated_gives_the_root_and_rows_of_commit(sb, oracle, kind):
    from stark_brainfuck_amd.device import DeviceBuffer
    N, d, count = 256, 64, 3
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    pc = sb.PolynomialCommitment(sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, 4, 2, XF))
    if kind == "extension":
        polys = [sb.XArray.from_numpy(oracle.felt_array(0xDEE9, 100 * k, 3 * (d - k)).reshape(3, d - k), XF) for k in range(count)]
        codewords = np.concatenate([pc.fri.domain.xevaluate(f, as_array=True).to_numpy().reshape(-1) for f in polys])
    else:
        polys = [sb.BaseArray.from_numpy(oracle.felt_array(0xDEE9, 100 * k, d - k)) for k in range(count)]
        codewords = np.concatenate([pc.fri.domain.evaluate(f, as_array=True).to_numpy().reshape(-1) for f in polys])
    ps, ps_evaluated = sb.ProofStream(), sb.ProofStream()
    committed = pc.commit(polys, ps)
    buffer = DeviceBuffer.from_numpy(codewords)
    evaluated = pc.commit_evaluated(polys, buffer, ps_evaluated)
    assert evaluated.codewords is buffer and np.array_equal(buffer.to_numpy(), codewords)          # kept, not copied, not written
    assert np.array_equal(committed.codewords.to_numpy(), codewords)
    assert evaluated.root() == committed.root() and ps.objects == ps_evaluated.objects == [committed.root()]
    assert (evaluated.n_ext, evaluated.n_base, evaluated.order) == (committed.n_ext, committed.n_base, committed.order)
    assert [evaluated.tree.open(i) for i in (0, 1, 77, N - 1)] == [committed.tree.open(i) for i in (0, 1, 77, N - 1)]
    # ... and an opening through either commitment is the same bytes
    z = [XF.from_limbs([5, 6, 7])]
    values = pc.open(committed, z, ps)
    assert [[tuple(v.limbs()) for v in per_point] for per_point in pc.open(evaluated, z, ps_evaluated)] == [[tuple(v.limbs()) for v in per_point] for per_point in values]
    assert ps.serialize() == ps_evaluated.serialize()


# ------------------------------------------------------------------------------------------------ 3. end to end
CASES = [(name, mode()) for name in NAMES] + [("two_io", deep.MODE_A8C_G4)]
IDS = [deep.fixture_file(name, m)[len("deep_"):-len("_proof.bin")] for name, m in CASES]


@pytest.mark.parametrize("name,m", CASES, ids=IDS)
def test_verify_deep_accepts_prove_deep_and_the_bytes_are_the_fixtures(sb, name, m):
    stark, proof = proved(name, m)
    assert (stark.fri.folding_factor, stark.fri.coset_leaves, stark.fri.grinding_bits) == (m["folding_factor"], m["coset_leaves"], m["grinding_bits"])
    assert deep.make_stark(name, m).verify_deep(proof) is True
    entry = next(e for e in deep.fixtures() if e["file"] == deep.fixture_file(name, m))
    committed = open(os.path.join(GOLDEN, entry["file"]), "rb").read()
    assert hashlib.sha256(committed).hexdigest() == entry["proof_sha256"] and (entry["program"], entry["input"]) == deep.PROGRAMS[name]
    assert proof == committed
    assert sorted(stark.timing) == sorted(["pad", "base_lde", "base_commit", "extend", "ext_lde", "ext_commit", "composition", "composition_commit",
                                           "opening", "serialize"])


def test_the_debug_switch_checks_the_degree_of_the_composition_on_the_full_domain(sb, monkeypatch):
    """BFS_DEBUG=1: H on all N points interpolates to N / expansion_factor coefficients for an honest trace (the same proof bytes), and
    does not for a false one (without the switch the prover goes on and verify_deep refuses the proof)"""
    from stark_brainfuck_amd.vm import LazyTraceMatrix, VirtualMachine
    monkeypatch.setenv("BFS_DEBUG", "1")
    assert deep.prove_deep_seeded("loop")[1] == proved("loop")[1]
    matrices = list(deep.claim("loop")[4])
    values = np.array(matrices[0].values, dtype=np.uint64)
    values[1, 5] = (int(values[1, 5]) + 1) % _xfe().P
    with pytest.raises(AssertionError, match="composition polynomial has degree"):
        deep.prove_deep_seeded("loop", matrices=[LazyTraceMatrix(np.ascontiguousarray(values), VirtualMachine.field)] + matrices[1:])


def _plus1_fixture():
    return open(os.path.join(GOLDEN, deep.fixture_file("plus1", mode())), "rb").read()


def test_the_unsegmented_proof_keeps_its_one_segment_and_commits_to_the_working_codewords(sb):
    """BrainfuckStark.deep_shape: the mode is the one-segment case -- the segment is H's coefficients, nothing is decimated"""
    stark, proof = proved("plus1")
    last, shape = stark._last, stark.deep_shape()
    assert (last["L"], last["S"], last["s"]) == (shape.L, shape.S, 1) and shape.S == stark.max_degree + 1 == deep.DOMAINS["plus1"] // 4
    assert len(last["segments"]) == 1 and last["plan"].widths == (16, 9, 1)
    assert last["segments"][0].to_numpy().shape == (3, shape.S) and np.array_equal(last["segments"][0].to_numpy(), last["h_coefficients"].to_numpy())
    assert last["committed_base_codewords"] is last["working_base_codewords"] and last["committed_ext_codewords"] is last["working_ext_codewords"]
    assert last["commitments"][0].codewords is last["working_base_codewords"] and [c.n for c in last["commitments"]] == [shape.n] * 3
    assert proof == _plus1_fixture()


def test_the_debug_switch_leaves_the_unsegmented_bytes_of_plus1(sb, monkeypatch):
    """BFS_DEBUG=1 on a claim with empty input and output tables: the degree check and the assertion that the segments tile H (one
    segment here) hold for the honest trace, and the proof is the fixture"""
    monkeypatch.setenv("BFS_DEBUG", "1")
    assert deep.prove_deep_seeded("plus1")[1] == _plus1_fixture()


def test_every_fixture_is_proven_here():
    assert sorted(e["file"] for e in deep.fixtures()) == sorted(deep.fixture_file(name, m) for name, m in CASES)


def _horner(coefficients, z):
    air = _xfe()
    acc = air.X0
    for c in reversed(coefficients):
        acc = air.xadd(air.xmul(acc, z), c)
    return acc


@pytest.mark.parametrize("name", NAMES)
def test_the_opened_values_are_the_polynomials_values(sb, name):
    """Horner in Python integers over the kept coefficient buffers, at most height + 1 coefficients each, at z and z * omicron; H over its
    N / expansion_factor coefficients at z"""
    air = _xfe()
    stark, _ = proved(name)
    last = stark._last
    z, plan, opened = last["z"], last["plan"], last["opened"]
    coefficients = []
    for f in last["base_polys"]:
        coefficients.append([(int(v), 0, 0) for v in f.to_numpy()])
    for f in last["ext_polys"] + [last["h_coefficients"]]:
        coefficients.append([tuple(int(v) for v in c) for c in f.to_numpy().T])
    owners = [t for t in stark.tables for _ in range(t.base_width)] + [t for t in stark.tables for _ in range(t.full_width - t.base_width)]
    assert [len(c) for c in coefficients[:-1]] == [t.height + t.num_randomizers if t.height else 1 for t in owners]
    assert len(coefficients[-1]) == stark.fri.domain.length // stark.expansion_factor
    assert len(plan.groups) == len(opened)
    for (columns, points), per_group in zip(plan.groups, opened):
        assert len(points) == len(per_group)
        for point, per_point in zip(points, per_group):
            assert per_point == [_horner(coefficients[c], point) for c in columns]
    # the points: z and, for a table of height above 1, z times its subgroup generator
    for t, g in zip(stark.tables, plan.table_group):
        if g is not None:
            assert plan.groups[g][1] == ([z] if t.height == 1 else [z, air.xscale(z, t.omicron.value)])


@pytest.mark.parametrize("name", NAMES)
def test_the_identity_holds_through_the_mpolynomial_presentation(sb, name):
    """the left-hand side of the verifier's equation from Table._constraints_ext (pinned against the reference by existing tests),
    evaluated at the opened values, equals the opened H(z)"""
    air = _xfe()
    stark, _ = proved(name)
    last = stark._last
    XF = stark.xfield
    z, plan, opened = last["z"], last["plan"], last["opened"]
    challenges = [XF.from_limbs(list(c)) for c in last["challenges"]]
    terminals = [XF.from_limbs(list(t)) for t in last["terminals"]]
    weights = [tuple(int(v) for v in w) for w in last["weights"]]
    boundary = air.xinv(air.xsub(z, air.X1))
    total, at, rows = air.X0, 0, []
    for t, g in zip(stark.tables, plan.table_group):
        if g is None:
            rows.append([air.X0] * t.full_width)
            at += t.num_quotients()
            continue
        cur = opened[g][0]
        nxt = opened[g][1] if len(opened[g]) > 1 else cur
        rows.append(cur)
        off = air.xsub(z, (pow(t.omicron.value, air.P - 2, air.P), 0, 0))
        factors = {"boundary": boundary, "transition": air.xmul(off, air.xinv(air.xsub(air.xpow(z, t.height), air.X1))), "terminal": air.xinv(off)}
        for kind in ("boundary", "transition", "terminal"):
            point = [XF.from_limbs(list(v)) for v in (cur + nxt if kind == "transition" else cur)]
            for constraint in t._constraints_ext(kind, challenges, terminals if kind == "terminal" else None):
                value = tuple(constraint.evaluate(point).limbs()) if not constraint.is_zero() else air.X0
                value = value + (0,) * (3 - len(value))
                total = air.xadd(total, air.xmul(air.xmul(weights[at], value), factors[kind]))
                at += 1
    for j, pa in enumerate(stark.permutation_arguments):
        total = air.xadd(total, air.xmul(air.xmul(weights[at + j], pa.evaluate_difference(rows)), boundary))
    assert at + 2 == len(weights) == 50
    assert total == opened[plan.h_group][0][0]


# ------------------------------------------------------------------------------------------------ 4. refusals
def _refused(stark, proof, capsys):
    capsys.readouterr()
    verdict = stark.verify_deep(proof)
    printed = capsys.readouterr().out
    assert printed.count("\n") == 1, "a refusal prints one line: %r" % printed
    return verdict


@pytest.mark.parametrize("name", ["io", "loop"])
def test_false_traces_other_claims_and_tampered_proofs_are_refused(sb, name, capsys):
    from stark_brainfuck_amd.vm import LazyTraceMatrix, VirtualMachine
    stark, proof = proved(name)
    verifier = deep.make_stark(name)
    assert verifier.verify_deep(proof) is True
    # a trace with one processor cell changed: the prover still returns bytes
    matrices = list(deep.claim(name)[4])
    values = np.array(matrices[0].values, dtype=np.uint64)
    values[1, 5] = (int(values[1, 5]) + 1) % _xfe().P          # the memory value of the second cycle
    processor = LazyTraceMatrix(np.ascontiguousarray(values), VirtualMachine.field)
    false_proof = deep.prove_deep_seeded(name, matrices=[processor] + matrices[1:])[1]
    assert isinstance(false_proof, bytes) and false_proof != proof
    verdicts = {"a false trace": _refused(verifier, false_proof, capsys)}
    other = deep.make_stark(name, output_symbols=[chr(ord(deep.claim(name)[3][0]) + 1)])
    verdicts["another output symbol"] = _refused(other, proof, capsys)
    for what, data in deep.tamperings(proof).items():
        verdicts[what] = _refused(verifier, data, capsys)
    program, _, _, _, traces = deep.claim(name)
    verdicts["a proof of prove"] = _refused(verifier, deep.make_stark(name).prove(program, *traces), capsys)
    assert verdicts == {what: False for what in verdicts} and len(verdicts) == 7
    assert verifier.verify_deep(proof) is True
