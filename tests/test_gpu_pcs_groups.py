"""Opening each committed polynomial at its own set of points on the MI355X: the two entries of include/bfstark_open.h against the
CPython model (tests/pcs_groups_model.py), what they leave alone (tests/painted.py), the stream they keep to
(tests/pcs_groups_stream_child.py), their exports, and PolynomialCommitment.open_at / verify_at end to end: proof bytes equal to the
model's, both verifiers.  Exact integer arithmetic: every comparison is for equality."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import pcs_groups_cases as cases
import pcs_groups_model as gmodel
import pcs_model as model
import stark_fri_modes_streams as streams
from painted import Arena

pytestmark = pytest.mark.gpu

P = model.P
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_SECONDS = 120
u64, u32 = ctypes.c_uint64, ctypes.c_uint32


@pytest.fixture(scope="module")
def sb():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import stark_brainfuck_amd
    return stark_brainfuck_amd


@pytest.fixture(scope="module")
def lib(sb):
    from stark_brainfuck_amd import _lib
    return _lib.load()


def _flat(triples):
    return (u64 * (3 * len(triples)))(*[int(v) for z in triples for v in z])


def _upload(words):
    from stark_brainfuck_amd.device import DeviceBuffer
    return DeviceBuffer.from_numpy(np.ascontiguousarray(words, dtype=np.uint64).reshape(-1))


# ------------------------------------------------------------------------------------------------ 1. evaluation of separate columns
@pytest.mark.parametrize("name", sorted(cases.EVAL_CASES))
@pytest.mark.parametrize("k", cases.EVAL_POINT_COUNTS)
def test_evaluation_of_separate_columns_is_the_models(sb, lib, name, k):
    """every column in an allocation of its own; the output in a painted arena, the inputs read back"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import current_stream
    columns, points, reference = cases.eval_case(name)
    buffers = [_upload(c) for c in columns]
    table = (_lib.EvalColumn * len(columns))(*[_lib.EvalColumn(buf.ptr, c.size) for buf, c in zip(buffers, columns)])
    arena = Arena(batch=1, n=3 * len(columns) * k)
    _lib.check(lib.bfsx_poly_eval_columns(table, len(columns), _flat(points[:k]), k, arena.ptr, current_stream()))
    after = arena.contained([("column %d" % b, c, buf.to_numpy()) for b, (buf, c) in enumerate(zip(buffers, columns))])
    out = arena.rows(after)[0]
    got = [[tuple(int(v) for v in out[(b * k + j) * 3:(b * k + j) * 3 + 3]) for j in range(k)] for b in range(len(columns))]
    assert got == [row[:k] for row in reference]


def test_evaluation_refuses_bad_arguments(sb, lib):
    from stark_brainfuck_amd import _lib
    src, out = _upload(np.zeros(16)), _upload(np.zeros(3 * 97 * 4))
    pts = _flat([(1, 2, 3)])

    def table(entries):
        return (_lib.EvalColumn * len(entries))(*[_lib.EvalColumn(ptr, n) for ptr, n in entries])
    one = table([(src.ptr, 8)])
    assert lib.bfsx_poly_eval_columns(one, 1, pts, 1, out.ptr, None) == 0
    bad = [(one, 0, pts, 1, out.ptr), (table([(src.ptr, 8)] * 97), 97, pts, 1, out.ptr), (one, 1, pts, 0, out.ptr), (one, 1, pts, 5, out.ptr),
           (table([(src.ptr, 8), (src.ptr, 0)]), 2, pts, 1, out.ptr), (table([(src.ptr, (1 << 24) + 1)]), 1, pts, 1, out.ptr),
           (table([(src.ptr, 8), (None, 8)]), 2, pts, 1, out.ptr), (one, 1, _flat([(P, 0, 0)]), 1, out.ptr), (one, 1, pts, 1, src.ptr + 8),
           (table([(out.ptr, 8), (src.ptr + 40, 8)]), 2, pts, 1, src.ptr)]          # (the output's last word lies in the second column)
    assert [lib.bfsx_poly_eval_columns(*args, None) for args in bad] == [6] * len(bad)


# ------------------------------------------------------------------------------------------------ 2. the quotient of a plan
def _quotient_call(case, buffers, out_ptr, out_stride, stream):
    """the argument list of bfsx_deep_quotient_groups for a case whose row columns lie in `buffers`"""
    from stark_brainfuck_amd import _lib
    args = cases.kernel_arguments(case)
    cols = (_lib.RowColumn * len(args["order"]))()
    for at, c in enumerate(args["order"]):
        cols[at].d_values, cols[at].is_ext, cols[at].field_id = buffers[c].ptr, int(case["columns"][c].ndim == 2), 1
    groups, pairs = len(args["group_columns"]), len(args["pair_point"])
    return [cols, len(args["order"]), case["stride"], case["N"].bit_length() - 1, cases.OFFSET, case["omega"], (u32 * groups)(*args["group_columns"]),
            (u32 * groups)(*args["group_pairs"]), groups, _flat(args["points"]), len(args["points"]), (u32 * pairs)(*args["pair_point"]),
            _flat(args["pair_values"]), (u64 * 3)(*case["lam"]), out_ptr, out_stride, stream]


def _quotient(lib, case, out_stride):
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import current_stream
    buffers = [_upload(c) for c in case["columns"]]
    arena = Arena(batch=3, stride=out_stride, n=case["N"])
    _lib.check(lib.bfsx_deep_quotient_groups(*_quotient_call(case, buffers, arena.ptr, out_stride, current_stream())))
    after = arena.contained([("codeword %d" % p, np.ascontiguousarray(c).reshape(-1), buf.to_numpy()) for p, (buf, c) in enumerate(zip(buffers, case["columns"]))])
    return arena.rows(after), buffers


@pytest.mark.parametrize("N", cases.QUOTIENT_SIZES)
@pytest.mark.parametrize("layout", sorted(cases.LAYOUTS))
@pytest.mark.parametrize("k", cases.POINT_COUNTS)
def test_one_group_of_all_columns_is_bfs_deep_quotient_word_for_word(sb, lib, N, layout, k):
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import current_stream
    case = cases.plan_one(N, layout, k, stride=N + 24)
    got, buffers = _quotient(lib, case, N + 40)
    assert np.array_equal(got, case["g"])
    cols = (_lib.RowColumn * len(buffers))()
    for p, (buf, c) in enumerate(zip(buffers, case["columns"])):
        cols[p].d_values, cols[p].is_ext, cols[p].field_id = buf.ptr, int(c.ndim == 2), 1
    old = Arena(batch=3, stride=N + 40, n=N)
    _lib.check(lib.bfs_deep_quotient(cols, len(buffers), case["stride"], N.bit_length() - 1, cases.OFFSET, case["omega"], _flat(case["plan"].points),
                                     _flat(case["Y"][0]), k, (u64 * 3)(*case["lam"]), old.ptr, N + 40, current_stream()))
    assert np.array_equal(old.rows(old.contained()), got)


@pytest.mark.parametrize("N", cases.QUOTIENT_SIZES)
def test_tables_plan_is_the_models(sb, lib, N):
    assert np.array_equal(_quotient(lib, cases.plan_tables(N, stride=N + 24), N + 40)[0], cases.plan_tables(N, stride=N + 24)["g"])


@pytest.mark.parametrize("N", cases.MAX_SIZES)
def test_plan_at_every_limit_is_the_models(sb, lib, N):
    assert np.array_equal(_quotient(lib, cases.plan_max(N, stride=N + 24), N + 40)[0], cases.plan_max(N, stride=N + 24)["g"])


@pytest.mark.parametrize("N", cases.QUOTIENT_SIZES)
def test_singletons_are_one_group_at_one_point(sb, lib, N):
    case = cases.plan_singletons(N, stride=N + 24)
    assert case["g"] is cases.plan_one(N, "mixed", 1, stride=N + 24)["g"]
    assert np.array_equal(_quotient(lib, case, N + 40)[0], case["g"])


def test_quotient_refuses_bad_arguments(sb, lib):
    N = 64
    case = cases.plan_tables(N)
    buffers = [_upload(c) for c in case["columns"]]
    out = _upload(np.zeros(3 * N))
    good = _quotient_call(case, buffers, out.ptr, N, None)
    assert [list(good[6]), list(good[7]), good[8], good[10], list(good[11])] == [[3, 2, 2], [2, 2, 1], 3, 3, [0, 1, 0, 2, 0]]

    def rc(**change):
        args = list(good)
        for at, value in change.items():
            args[int(at[1:])] = value
        return lib.bfsx_deep_quotient_groups(*args)
    nine = (u32 * 9)(*[1] * 9)
    refused = {"no column": rc(a1=0), "33 columns": rc(a1=33), "no group": rc(a8=0), "9 groups": rc(a6=nine, a7=nine, a8=9), "no point": rc(a10=0),
               "9 points": rc(a10=9), "log_n 0": rc(a3=0), "log_n 25": rc(a3=25), "a short limb stride": rc(a2=N - 1), "a short output stride": rc(a15=N - 1),
               "offset 0": rc(a4=0), "sizes that sum to 6": rc(a6=(u32 * 3)(3, 2, 1)), "sizes that sum to 8": rc(a6=(u32 * 3)(3, 2, 3)),
               "an empty group": rc(a6=(u32 * 3)(3, 0, 4)), "a group without a pair": rc(a7=(u32 * 3)(2, 0, 3)),
               "five pairs in a group": rc(a7=(u32 * 3)(5, 1, 1), a11=(u32 * 7)(0, 1, 2, 0, 1, 0, 0)),
               "17 pairs": rc(a1=5, a6=(u32 * 5)(*[1] * 5), a7=(u32 * 5)(4, 4, 4, 4, 1), a8=5, a11=(u32 * 17)(*([0, 1, 2, 0] * 4 + [0])), a12=_flat([(1, 2, 3)] * 17)),
               "a pair index of 3": rc(a11=(u32 * 5)(0, 1, 0, 3, 0)), "a point twice in a group": rc(a11=(u32 * 5)(0, 1, 2, 2, 0)),
               "an unreduced point": rc(a9=_flat([(P, 0, 0)] * 3)), "an unreduced value": rc(a12=_flat([(1, P, 0)] * 5)), "an unreduced lambda": rc(a13=(u64 * 3)(1, 2, P)),
               "output over a codeword": rc(a14=buffers[0].ptr)}
    assert rc() == 0
    assert refused == {name: 6 for name in refused}
    assert rc(a5=case["omega"] * case["omega"] % P) == 2          # BFS_ERR_NOT_ROOT


def test_points_in_another_order_and_an_unused_point_change_no_word(sb, lib, oracle):
    """the entry gives a launch the points its pairs name, in order of first appearance: the plan's points in another order, or with a
    point that no pair names behind them, give the same words (field arithmetic is exact) and nothing beside them.  An unused point
    is still checked: unreduced, it is refused"""
    from stark_brainfuck_amd.device import current_stream
    N = 64
    case = cases.plan_tables(N)
    buffers = [_upload(c) for c in case["columns"]]
    points, pair_point = list(case["plan"].points), cases.kernel_arguments(case)["pair_point"]
    assert len(points) == 3 and pair_point == [0, 1, 0, 2, 0]

    def call(points, pair_point):
        arena = Arena(batch=3, stride=N + 40, n=N)
        args = _quotient_call(case, buffers, arena.ptr, N + 40, current_stream())          # (pair_values stay: the pairs keep their order)
        args[9], args[10], args[11] = _flat(points), len(points), (u32 * len(pair_point))(*pair_point)
        return lib.bfsx_deep_quotient_groups(*args), arena
    order = [2, 0, 1]                                 # place i of the permuted array holds point order[i]
    spare = cases.random_points(oracle, 4242, 1)[0]
    assert spare not in points and all(v < P for v in spare)
    for other_points, other_pairs in (([points[p] for p in order], [order.index(p) for p in pair_point]), (points + [spare], pair_point)):
        rc, arena = call(other_points, other_pairs)
        assert rc == 0
        assert np.array_equal(arena.rows(arena.contained()), case["g"])
    rc, arena = call(points + [(P, 0, 0)], pair_point)
    assert rc == 6
    assert np.array_equal(arena.contained(), arena.image)          # a refused call enqueues nothing


# ------------------------------------------------------------------------------------------------ 3. stream order
def test_both_entries_keep_to_their_stream(sb):
    """tests/pcs_groups_stream_child.py, once, in a child process under its own time limit"""
    proc = subprocess.run([sys.executable, os.path.join(HERE, "pcs_groups_stream_child.py")], capture_output=True, text=True, timeout=CHILD_SECONDS)
    lines = [json.loads(l) for l in proc.stdout.splitlines() if l.startswith("{")]
    for l in lines:
        print(json.dumps(l))
    errors = [l["error"] for l in lines if "error" in l]
    assert proc.returncode == 0 and not errors and lines and lines[-1].get("done"), "the child ended with status %s: %s\n%s" % (
        proc.returncode, errors, proc.stderr[-2000:])
    assert [l["ok"] for l in lines if "control" in l] == [True]
    by_case = {l["case"]: l for l in lines if "case" in l}
    assert sorted(by_case) == ["deep_quotient_groups", "poly_eval_columns"]
    for name, line in by_case.items():
        assert line["kind"] == "enqueues" and line["ok"], "%s: %s" % (name, "\n".join(line["failures"]))


# ------------------------------------------------------------------------------------------------ 4. exports
def test_the_library_exports_what_the_header_declares(sb, lib):
    from stark_brainfuck_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "bfstark_open.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bfsx_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("bfsx_")}
    assert declared == exported == set(_lib.open_exported_symbols()) == {"bfsx_poly_eval_columns", "bfsx_deep_quotient_groups"}
    assert all(getattr(lib, name).argtypes for name in declared)
    # every stream-taking function of the header is a case of the child above
    taking = set(re.findall(r"\b(bfsx_[a-z0-9_]+)\s*\([^;]*void\*\s*stream\)", text))
    import pcs_groups_stream_child as child
    assert taking == declared == {e for c in (child.eval_case(), child.quotient_case()) for e in c.entries}


# ------------------------------------------------------------------------------------------------ 5. end to end
PROTOCOL = [(N, mode) for mode in ("default", "fold4", "coset8") for N in (256, 1024)]
IDS = ["%d-%s" % c for c in PROTOCOL]


def _fri(sb, N, mode):
    a, coset, bits = cases.MODES[mode]
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    return sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, cases.EXPANSION, cases.T, XF, folding_factor=a, coset_leaves=coset, grinding_bits=bits)


@pytest.mark.parametrize("N,mode", PROTOCOL, ids=IDS)
def test_proof_bytes_are_the_models_and_both_verifiers_accept(sb, lib, oracle, N, mode):
    import test_pcs_host as host
    proof = cases.model_proof(N, mode)
    a, coset, _ = cases.MODES[mode]
    pc = sb.PolynomialCommitment(_fri(sb, N, mode))
    ext = [sb.XArray.from_numpy(f, pc.xfield) for f in proof["ext"]]
    base = [sb.BaseArray.from_numpy(f) for f in proof["base"]]
    polys = [base[0], ext[0], base[1], base[2], ext[1]]          # (the caller's order is not the row's)
    ps = sb.ProofStream()
    committed = pc.commit(polys, ps)
    assert committed.order == [1, 4, 0, 2, 3] and [committed.column_of(p) for p in range(5)] == [2, 0, 3, 4, 1]
    assert committed.root() == proof["root"]
    values = pc.open_at(committed, proof["raw_plan"], ps)
    limbs = [[[tuple(v.limbs()) for v in per_point] for per_point in per_group] for per_group in values]
    assert limbs == proof["values"]
    data = ps.serialize()
    assert data == proof["bytes"]
    # the values are evaluate_at's
    plan = proof["plan"]
    for (columns, indices), per_group in zip(plan.groups, limbs):
        for p, per_point in zip(indices, per_group):
            z = pc.xfield.from_limbs(list(plan.points[p]))
            assert per_point == [tuple(sb.evaluate_at(polys[committed.order[c]], [z])[0].limbs()) for c in columns]
    back = sb.ProofStream().deserialize(data)
    back.pull()
    assert pc.verify_at(committed.root(), proof["raw_plan"], values, back) is True
    assert gmodel.verify(oracle, streams.load(oracle, data), committed.root(), proof["raw_plan"], limbs, N, cases.OFFSET, proof["omega"], cases.T, a, coset,
                         host._fri_verify(sb, N, mode)) == (True, "accepted")


def test_a_bad_plan_is_refused_with_a_commitment_in_hand(sb):
    N = 256
    pc = sb.PolynomialCommitment(_fri(sb, N, "default"))
    ps = sb.ProofStream()
    committed = pc.commit([sb.BaseArray.from_numpy(np.arange(1, 9, dtype=np.uint64)), sb.BaseArray.from_numpy(np.arange(2, 7, dtype=np.uint64))], ps)
    for plan in ([([0], [(1, 2, 3)])], [([0, 1], [(cases.OFFSET, 0, 0)])], [([0, 1], [(1, 2, 3)]), ([1], [(1, 2, 4)])]):
        with pytest.raises(ValueError):
            pc.open_at(committed, plan, ps)
    assert len(ps.objects) == 1
