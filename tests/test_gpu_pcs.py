"""Opening committed polynomials at out-of-domain points on the MI355X: the two kernels of csrc/deep.hip against the CPython model
(tests/pcs_model.py), what they leave alone (tests/painted.py), the stream they keep to (tests/pcs_stream_child.py: the two legs of
tests/stream_order_child.py), the exports of include/bfstark_ext.h, and PolynomialCommitment end to end: proof bytes equal to the
model's, both verifiers, the refusals.  Exact integer arithmetic: every comparison is for equality."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import pcs_cases as cases
import pcs_model as model
import stark_fri_modes_streams as streams
from painted import Arena

pytestmark = pytest.mark.gpu

P = model.P
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_SECONDS = 120
u64 = ctypes.c_uint64


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


def _upload(sb, words):
    from stark_brainfuck_amd.device import DeviceBuffer
    return DeviceBuffer.from_numpy(np.ascontiguousarray(words, dtype=np.uint64).reshape(-1))


# ------------------------------------------------------------------------------------------------ 1. evaluation
def _evaluate(sb, lib, coeffs, n, stride, batch, points):
    """-> (values[b][j], the arena's snapshot check done): the output in a painted arena, the input read back"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import current_stream
    k = len(points)
    src = _upload(sb, coeffs)
    arena = Arena(batch=1, n=3 * batch * k)
    _lib.check(lib.bfs_poly_eval_points(src.ptr, n, stride, batch, _flat(points), k, arena.ptr, current_stream()))
    after = arena.contained([("coefficients", np.ascontiguousarray(coeffs).reshape(-1), src.to_numpy())])
    out = arena.rows(after)[0]
    return [[tuple(int(v) for v in out[(b * k + j) * 3:(b * k + j) * 3 + 3]) for j in range(k)] for b in range(batch)]


@pytest.mark.parametrize("n", cases.EVAL_LENGTHS)
def test_evaluation_is_the_models(sb, lib, n):
    coeffs, points, reference = cases.eval_case(n)
    for batch, k in cases.eval_shapes(n):
        got = _evaluate(sb, lib, coeffs[:batch], n, coeffs.shape[1], batch, points[:k])
        assert got == [[reference[b][j] for j in range(k)] for b in range(batch)], (n, batch, k)


@pytest.mark.parametrize("n,stride", [((1 << 16) + 3, (1 << 16) + 3), (100003, 100003 + 61), (65, 80)])
def test_evaluation_over_several_workgroups_with_a_ragged_tail_and_a_stride(sb, lib, n, stride):
    """2^16 + 3: five workgroups, three coefficients in the last; 100 003 with a stride: seven, junk between the columns"""
    coeffs, points, reference = cases.eval_case(n, stride)
    batch, k = (3, 2) if n <= 1000 else (1, 1)
    got = _evaluate(sb, lib, coeffs[:batch + 1], n, stride, batch, points[:k])          # (one column more than the call reads lies behind)
    assert got == [[reference[b][j] for j in range(k)] for b in range(batch)]


def test_evaluation_refuses_bad_arguments(sb, lib):
    src, out = _upload(sb, np.zeros(16)), _upload(sb, np.zeros(64))
    pts = _flat([(1, 2, 3)])
    bad = [(src.ptr, 0, 8, 1, pts, 1, out.ptr), (src.ptr, 8, 8, 1, pts, 0, out.ptr), (src.ptr, 8, 8, 1, pts, 5, out.ptr),
           (src.ptr, 8, 4, 2, pts, 1, out.ptr), (src.ptr, (1 << 24) + 1, 8, 1, pts, 1, out.ptr), (src.ptr, 8, 8, 1, _flat([(P, 0, 0)]), 1, out.ptr),
           (src.ptr, 8, 8, 1, pts, 1, src.ptr + 8)]
    assert [lib.bfs_poly_eval_points(*args, None) for args in bad] == [6] * len(bad)


# ------------------------------------------------------------------------------------------------ 2. quotient
def _quotient(sb, lib, case, N, k, out_stride):
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import current_stream
    stride = case["stride"]
    buffers = [_upload(sb, c) for c in case["columns"]]
    cols = (_lib.RowColumn * len(buffers))()
    for p, (buf, c) in enumerate(zip(buffers, case["columns"])):
        cols[p].d_values, cols[p].is_ext, cols[p].field_id = buf.ptr, int(c.ndim == 2), 1
    arena = Arena(batch=3, stride=out_stride, n=N)
    _lib.check(lib.bfs_deep_quotient(cols, len(buffers), stride, N.bit_length() - 1, cases.OFFSET, case["omega"], _flat(case["points"]),
                                     _flat(case["values"]), k, (u64 * 3)(*case["lam"]), arena.ptr, out_stride, current_stream()))
    after = arena.contained([("codeword %d" % p, np.ascontiguousarray(c).reshape(-1), buf.to_numpy()) for p, (buf, c) in enumerate(zip(buffers, case["columns"]))])
    return arena.rows(after)


@pytest.mark.parametrize("N", cases.QUOTIENT_SIZES + (1 << 12,))
@pytest.mark.parametrize("layout", sorted(cases.LAYOUTS))
@pytest.mark.parametrize("k", cases.POINT_COUNTS)
def test_quotient_is_the_models_word_for_word(sb, lib, N, layout, k):
    case = cases.quotient_case(N, layout, k, stride=N + 24 if layout == "mixed" else None)
    assert np.array_equal(_quotient(sb, lib, case, N, k, N + 40), case["g"])


def test_quotient_at_2_16_mixed(sb, lib):
    N = 1 << 16
    case = cases.quotient_case(N, "mixed", 1)
    assert np.array_equal(_quotient(sb, lib, case, N, 1, N + 8), case["g"])


def test_quotient_refuses_bad_arguments(sb, lib):
    from stark_brainfuck_amd import _lib
    N = 64
    case = cases.quotient_case(N, "mixed", 2)
    buffers = [_upload(sb, c) for c in case["columns"]]
    out = _upload(sb, np.zeros(3 * N))
    cols = (_lib.RowColumn * len(buffers))()
    for p, (buf, c) in enumerate(zip(buffers, case["columns"])):
        cols[p].d_values, cols[p].is_ext, cols[p].field_id = buf.ptr, int(c.ndim == 2), 1
    pts, vals, lam = _flat(case["points"]), _flat(case["values"]), (u64 * 3)(*case["lam"])
    good = [cols, 5, N, 6, cases.OFFSET, case["omega"], pts, vals, 2, lam, out.ptr, N, None]

    def rc(**change):
        args = list(good)
        for at, value in change.items():
            args[int(at[1:])] = value
        return lib.bfs_deep_quotient(*args)
    assert rc() == 0
    assert [rc(a1=0), rc(a1=33), rc(a8=0), rc(a8=5), rc(a3=0), rc(a3=25), rc(a2=N - 1), rc(a11=N - 1), rc(a4=0), rc(a10=buffers[0].ptr)] == [6] * 10
    assert rc(a5=case["omega"] * case["omega"] % P) == 2          # BFS_ERR_NOT_ROOT


# ------------------------------------------------------------------------------------------------ 3. stream order
def test_both_entries_keep_to_their_stream(sb):
    """tests/pcs_stream_child.py, once, in a child process under its own time limit"""
    proc = subprocess.run([sys.executable, os.path.join(HERE, "pcs_stream_child.py")], capture_output=True, text=True, timeout=CHILD_SECONDS)
    lines = [json.loads(l) for l in proc.stdout.splitlines() if l.startswith("{")]
    for l in lines:
        print(json.dumps(l))
    errors = [l["error"] for l in lines if "error" in l]
    assert proc.returncode == 0 and not errors and lines and lines[-1].get("done"), "the child ended with status %s: %s\n%s" % (
        proc.returncode, errors, proc.stderr[-2000:])
    assert [l["ok"] for l in lines if "control" in l] == [True]
    by_case = {l["case"]: l for l in lines if "case" in l}
    assert sorted(by_case) == ["deep_quotient", "poly_eval_points"]
    for name, line in by_case.items():
        assert line["kind"] == "enqueues" and line["ok"], "%s: %s" % (name, "\n".join(line["failures"]))


# ------------------------------------------------------------------------------------------------ 4. exports
def _declared(header):
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(bfs_[a-z0-9_]+)\s*\(", text))


def test_the_library_exports_what_the_new_header_declares(sb, lib):
    from stark_brainfuck_amd import _lib
    new = _declared("bfstark_ext.h") - _declared("bfstark.h")
    assert new == {"bfs_poly_eval_points", "bfs_deep_quotient"} == set(_lib.ext_exported_symbols())
    assert not set(_lib.ext_exported_symbols()) & set(_lib.exported_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("bfs_")}
    assert exported - _declared("bfstark.h") == new
    # every stream-taking function of the new header is a case of the child above
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "bfstark_ext.h")).read(), flags=re.S)
    taking = set(re.findall(r"\b(bfs_[a-z0-9_]+)\s*\([^;]*void\*\s*stream\)", text))
    import pcs_stream_child
    assert taking == new == {e for c in (pcs_stream_child.eval_case(), pcs_stream_child.quotient_case()) for e in c.entries}


# ------------------------------------------------------------------------------------------------ 5. end to end
PROTOCOL = [(256, "default"), (1024, "default"), (256, "fold4"), (1024, "fold4"), (256, "coset8"), (1024, "coset8")]
IDS = ["%d-%s" % c for c in PROTOCOL]


def _fri(sb, N, mode):
    a, coset, bits = cases.MODES[mode]
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    return sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, cases.EXPANSION, cases.T, XF, folding_factor=a, coset_leaves=coset, grinding_bits=bits)


def _prove(sb, N, mode, proof):
    """commit and open the model's polynomials at the model's points -> (pc, proof bytes, root, values as limb triples)"""
    pc = sb.PolynomialCommitment(_fri(sb, N, mode))
    polys = [sb.XArray.from_numpy(f, pc.xfield) for f in proof["ext"]] + [sb.BaseArray.from_numpy(f) for f in proof["base"]]
    polys = polys[1:3] + polys[:1] + polys[3:]                      # (the caller's order is not the row's: base, base, ext, base)
    ps = sb.ProofStream()
    committed = pc.commit(polys, ps)
    assert committed.order == [2, 0, 1, 3]
    values = pc.open(committed, [pc.xfield.from_limbs(list(z)) for z in proof["points"]], ps)
    return pc, ps.serialize(), committed.root(), [[tuple(v.limbs()) for v in per] for per in values]


def _verdict(sb, N, mode, data, root, points, values, edit=None):
    pc = sb.PolynomialCommitment(_fri(sb, N, mode))
    ps = sb.ProofStream().deserialize(data)
    if edit is not None:
        ps.objects = edit(list(ps.objects))
    ps.pull()
    return pc.verify(root, [pc.xfield.from_limbs(list(z)) for z in points], [[pc.xfield.from_limbs(list(v)) for v in per] for per in values], ps)


@pytest.mark.parametrize("N,mode", PROTOCOL, ids=IDS)
@pytest.mark.parametrize("k", [1, 2])
def test_proof_bytes_are_the_models_and_both_verifiers_accept(sb, lib, oracle, N, mode, k):
    proof = cases.model_proof(N, mode, k, zero=(N == 256 and mode == "fold4"))
    coset = cases.MODES[mode][1]
    if coset:      # the seed is chosen so: no element of the model's g stores fewer than three coefficients (checked on the CPU)
        assert proof["g"][2].all()
    by_rows = lib.bfs_coset_trees_by_rows()
    pc, data, root, values = _prove(sb, N, mode, proof)
    assert lib.bfs_coset_trees_by_rows() == by_rows
    assert root == proof["root"]
    assert values == proof["values"]
    assert data == proof["bytes"]
    assert _verdict(sb, N, mode, data, root, proof["points"], values) is True
    import test_pcs_host as host
    a = cases.MODES[mode][0]
    objects = streams.load(oracle, data)
    assert model.verify(oracle, objects, root, proof["points"], values, N, cases.OFFSET, proof["omega"], cases.T, a, coset,
                        host._fri_verify(sb, N, mode)) == (True, "accepted")


@pytest.mark.parametrize("N,mode,seed,what", [(256, "default", 53, "shared"), (256, "fold4", 19, "shared"), (64, "default", 18, "repeated")])
def test_objects_that_recur_in_the_stream_are_the_same_objects(sb, N, mode, seed, what):
    """pickle writes a back-reference for an object it has seen.  shared: a consistency index is also an index FRI opens in round 0, so
    the element pushed with the row is the element of FRI's tuple (Fri.prove's known_leafs); repeated: the two consistency indices are
    equal, so row, element and digests recur.  The seeds were searched for on the CPU; the precondition is asserted here."""
    proof = cases.model_proof(N, mode, 1, seed=seed)
    a = cases.MODES[mode][0]
    q = N // a
    if what == "shared":
        assert set(proof["indices"]) & {c % q + j * q for c in proof["fri"]["indices"] for j in range(a)}
    else:
        assert proof["indices"][0] == proof["indices"][1]
    pc, data, root, values = _prove(sb, N, mode, proof)
    assert data == proof["bytes"]
    assert _verdict(sb, N, mode, data, root, proof["points"], values) is True


def test_a_point_given_twice_is_opened_twice(sb, oracle):
    """points = [z, z]: `open` does not refuse them (an OpeningPlan would), proves both, and `verify` accepts -- the bytes are the
    model's, which has no such rule either"""
    import test_pcs_host as host
    N, mode = 64, "default"
    proof = cases.model_proof(N, mode, 2, repeated=True)
    assert proof["points"][0] == proof["points"][1]
    pc, data, root, values = _prove(sb, N, mode, proof)
    assert values == proof["values"] and values[0] == values[1]
    assert data == proof["bytes"]
    assert _verdict(sb, N, mode, data, root, proof["points"], values) is True
    assert model.verify(oracle, streams.load(oracle, data), root, proof["points"], values, N, cases.OFFSET, proof["omega"], cases.T, 2, False,
                        host._fri_verify(sb, N, mode)) == (True, "accepted")


@pytest.mark.parametrize("N,mode", [(256, "default"), (256, "coset8")], ids=["256-default", "256-coset8"])
def test_tampered_streams_and_other_statements_are_refused(sb, N, mode):
    import test_pcs_host as host
    proof = cases.model_proof(N, mode, 2)
    pc, data, root, values = _prove(sb, N, mode, proof)
    points = proof["points"]
    verdicts = {"untouched": _verdict(sb, N, mode, data, root, points, values),
                "value": _verdict(sb, N, mode, data, root, points, values, edit=host._edit_value(sb)),
                "row": _verdict(sb, N, mode, data, root, points, values, edit=host._edit_row(sb)),
                "opening": _verdict(sb, N, mode, data, root, points, values, edit=host._edit_quotient_opening(sb, cases.MODES[mode][1])),
                "points": _verdict(sb, N, mode, data, root, [points[0], model.xadd(points[1], (1, 0, 0))], values),
                "root": _verdict(sb, N, mode, data, bytes(64), points, values)}
    assert verdicts == {"untouched": True, "value": False, "row": False, "opening": False, "points": False, "root": False}


def test_a_point_of_the_domain_is_refused_with_a_commitment_in_hand(sb):
    N = 256
    pc = sb.PolynomialCommitment(_fri(sb, N, "default"))
    ps = sb.ProofStream()
    committed = pc.commit([sb.BaseArray.from_numpy(np.arange(1, 9, dtype=np.uint64))], ps)
    before = len(ps.objects)
    with pytest.raises(ValueError):
        pc.open(committed, [pc.xfield.from_limbs([cases.OFFSET, 0, 0])], ps)
    assert len(ps.objects) == before == 1


# ------------------------------------------------------------------------------------------------ 6. evaluate_at
def test_evaluate_at_is_polynomial_evaluate_of_the_host_classes(sb, oracle):
    XF = sb.ExtensionField.main()
    internal = XF.modulus.coefficients[0].field
    n = 300
    base = oracle.felt_array(cases.SEED, 1, 2 * n).reshape(2, n)
    ext = oracle.felt_array(cases.SEED, 5000, 3 * n).reshape(3, n)
    points = [XF.from_limbs(list(z)) for z in cases.POINTS] + [XF.from_limbs([int(v) for v in oracle.felt_array(cases.SEED, 9000 + i, 3)]) for i in range(2)]

    def same(got, want):
        assert type(got) is sb.ExtensionFieldElement and got.field is XF and got.limbs() == want.limbs()
        assert all(type(c) is sb.BaseFieldElement and c.field is internal for c in got.polynomial.coefficients)
        assert len(got.polynomial.coefficients) == len(want.polynomial.coefficients)          # the stored form drops trailing zeros
    host_base = [sb.Polynomial([XF.from_limbs([int(v), 0, 0]) for v in row]) for row in base]
    host_ext = sb.Polynomial([XF.from_limbs([int(ext[0, i]), int(ext[1, i]), int(ext[2, i])]) for i in range(n)])
    one = sb.evaluate_at(sb.BaseArray.from_numpy(base[0]), points)
    both = sb.evaluate_at(sb.BaseArray.from_numpy(base), points)
    xs = sb.evaluate_at(sb.XArray.from_numpy(ext, XF), points)
    assert len(one) == len(both) == len(xs) == len(points) == 6          # (more than four points: two launches)
    for j, z in enumerate(points):
        same(one[j], host_base[0].evaluate(z))
        assert isinstance(both[j], list) and len(both[j]) == 2
        same(both[j][0], host_base[0].evaluate(z))
        same(both[j][1], host_base[1].evaluate(z))
        same(xs[j], host_ext.evaluate(z))
