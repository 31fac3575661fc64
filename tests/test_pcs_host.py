"""Opening committed polynomials at out-of-domain points (stark_brainfuck_amd/pcs.py, csrc/deep.hip), host side, no GPU: the verifier
against the proofs of a CPython model (tests/pcs_model.py), its refusals, the two kernels' per-thread code (csrc/deep_core.hpp through
tests/emu/emu_deep.cpp) against the model's arithmetic, the domain check.  Arithmetic is exact: every comparison is for equality."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

import pcs_cases as cases
import pcs_model as model

P = model.P
PROTOCOL = [(64, "default"), (256, "default"), (64, "fold4"), (256, "fold4"), (256, "coset8")]
IDS = ["%d-%s" % c for c in PROTOCOL]


@pytest.fixture(scope="session")
def sb():
    from stark_brainfuck_amd import build
    build.build_library()
    import stark_brainfuck_amd
    return stark_brainfuck_amd


@pytest.fixture(scope="module")
def emu():
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    from build_emu import build_emulation
    e = ctypes.CDLL(build_emulation())
    u64, vp = ctypes.c_uint64, ctypes.c_void_p
    e.emu_deep_eval.argtypes = [vp, u64, u64, ctypes.c_uint, vp, ctypes.c_uint, vp]
    e.emu_deep_quotient.argtypes = [vp, vp, ctypes.c_uint, u64, ctypes.c_uint, u64, u64, vp, vp, ctypes.c_uint, vp, vp, u64]
    return e


def _fri(sb, N, mode):
    a, coset, bits = cases.MODES[mode]
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    assert BF.generator().value == cases.OFFSET
    return sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, cases.EXPANSION, cases.T, XF, folding_factor=a, coset_leaves=coset, grinding_bits=bits)


def _elements(pc, triples):
    return [pc.xfield.from_limbs(list(z)) for z in triples]


def _package_verdict(sb, N, mode, data, root, points, values, edit=None):
    """PolynomialCommitment.verify on a serialised stream; edit(objects) -> objects tampers with the deserialised list"""
    pc = sb.PolynomialCommitment(_fri(sb, N, mode))
    ps = sb.ProofStream().deserialize(data)
    if edit is not None:
        ps.objects = edit(list(ps.objects))
    assert ps.pull() is not None                    # the commitment's root: the caller's to read
    return pc.verify(root, _elements(pc, points), [_elements(pc, per) for per in values], ps)


def _fri_verify(sb, N, mode):
    """the FRI layer's judge for the model's verifier: the package's host-side Fri.verify on the same objects"""
    from oracle import ref_oracle as o

    def judge(objects, read_index, g_root):
        ps = sb.ProofStream().deserialize(o.dumps(list(objects)))
        ps.read_index = read_index
        return _fri(sb, N, mode).verify(ps, g_root)
    return judge


def _model_verdict(sb, o, proof, root=None, points=None, values=None, objects=None):
    a, coset, _ = cases.MODES[proof["mode"]]
    return model.verify(o, proof["proof_stream"].objects if objects is None else objects, proof["root"] if root is None else root,
                        proof["points"] if points is None else points, proof["values"] if values is None else values, proof["N"], cases.OFFSET,
                        proof["omega"], cases.T, a, coset, _fri_verify(sb, proof["N"], proof["mode"]))


# ------------------------------------------------------------------------------------------------ 1. the model's own arithmetic
def test_model_arithmetic_is_the_oracles(oracle):
    values = cases.carry_values()
    triples = [(values[i % len(values)], values[(5 * i + 1) % len(values)], values[(7 * i + 2) % len(values)]) for i in range(40)]
    for a, b in zip(triples, triples[1:] + triples[:1]):
        assert list(model.xmul(a, b)) == oracle.xmul(a, b)
        if any(a):
            assert list(model.xinv(a)) == oracle.xinv(a)
            assert model.xmul(a, model.xinv(a)) == (1, 0, 0)
    assert list(model.xpow(triples[3], 12345)) == oracle.xpow(triples[3], 12345)


# ------------------------------------------------------------------------------------------------ 2. accept
@pytest.mark.parametrize("N,mode", PROTOCOL, ids=IDS)
@pytest.mark.parametrize("k", [1, 2])
def test_both_verifiers_accept_the_models_proof(sb, oracle, N, mode, k):
    proof = cases.model_proof(N, mode, k)
    assert _model_verdict(sb, oracle, proof) == (True, "accepted")
    assert _package_verdict(sb, N, mode, proof["bytes"], proof["root"], proof["points"], proof["values"]) is True


def test_a_zero_polynomial_is_opened(sb, oracle):
    proof = cases.model_proof(64, "default", 2, zero=True)
    assert all(v[3] == (0, 0, 0) for v in proof["values"])
    assert _package_verdict(sb, 64, "default", proof["bytes"], proof["root"], proof["points"], proof["values"]) is True


def test_a_point_given_twice_is_opened_twice(sb, oracle):
    """`open` and `verify` have no rule against points = [z, z] (an OpeningPlan has): two quotient terms over the same denominator,
    values[0] == values[1].  Both verifiers accept the model's proof; tests/test_gpu_pcs.py holds the prover to the same bytes"""
    proof = cases.model_proof(64, "default", 2, repeated=True)
    assert proof["points"][0] == proof["points"][1] and proof["values"][0] == proof["values"][1]
    assert _model_verdict(sb, oracle, proof) == (True, "accepted")
    assert _package_verdict(sb, 64, "default", proof["bytes"], proof["root"], proof["points"], proof["values"]) is True
    assert _package_verdict(sb, 64, "default", proof["bytes"], proof["root"], proof["points"][:1], proof["values"][:1]) is False      # (another statement)


# ------------------------------------------------------------------------------------------------ 3. refuse
def _bump(sb, element):
    limbs = element.limbs()
    return element.field.from_limbs([(limbs[0] + 1) % P, limbs[1], limbs[2] or 1])


def _edit_value(sb):
    def edit(objects):
        values = [list(per) for per in objects[2]]
        values[-1][0] = _bump(sb, values[-1][0])
        return objects[:2] + [values] + objects[3:]
    return edit


def _edit_row(sb):
    def edit(objects):
        assert isinstance(objects[4], tuple) and isinstance(objects[5], list)
        row = list(objects[4])
        row[0] = _bump(sb, row[0])
        return objects[:4] + [tuple(row)] + objects[5:]
    return edit


def _edit_quotient_opening(sb, coset):
    def edit(objects):
        leaf = objects[6]
        if coset:
            assert isinstance(leaf, tuple)
            leaf = tuple(_bump(sb, e) for e in leaf)
        else:
            leaf = _bump(sb, leaf)
        return objects[:6] + [leaf] + objects[7:]
    return edit


@pytest.mark.parametrize("N,mode", [(64, "default"), (256, "coset8")], ids=["64-default", "256-coset8"])
def test_the_verifier_refuses_tampered_streams_and_other_statements(sb, oracle, N, mode, capsys):
    proof = cases.model_proof(N, mode, 2)
    data, root, points, values = proof["bytes"], proof["root"], proof["points"], proof["values"]
    verdicts = {}
    verdicts["untouched"] = _package_verdict(sb, N, mode, data, root, points, values)
    verdicts["value"] = _package_verdict(sb, N, mode, data, root, points, values, edit=_edit_value(sb))
    verdicts["row"] = _package_verdict(sb, N, mode, data, root, points, values, edit=_edit_row(sb))
    verdicts["opening"] = _package_verdict(sb, N, mode, data, root, points, values, edit=_edit_quotient_opening(sb, cases.MODES[mode][1]))
    other_points = [points[0], model.xadd(points[1], (1, 0, 0))]
    verdicts["points"] = _package_verdict(sb, N, mode, data, root, other_points, values)
    other_values = [list(per) for per in values]
    other_values[0][2] = model.xadd(other_values[0][2], (0, 1, 0))
    verdicts["values"] = _package_verdict(sb, N, mode, data, root, points, other_values)
    verdicts["root"] = _package_verdict(sb, N, mode, data, bytes(64), points, values)
    forced = cases.model_proof(N, mode, 2, forced=True)
    assert forced["values"] != values
    verdicts["forced"] = _package_verdict(sb, N, mode, forced["bytes"], forced["root"], forced["points"], forced["values"])
    assert verdicts == {"untouched": True, "value": False, "row": False, "opening": False, "points": False, "values": False, "root": False,
                        "forced": False}
    printed = capsys.readouterr().out
    assert printed.count("\n") >= 7                    # one line per refusal, at least
    assert _model_verdict(sb, oracle, forced)[0] is False
    assert _model_verdict(sb, oracle, proof, root=bytes(64)) == (False, "root")
    assert _model_verdict(sb, oracle, proof, points=other_points) == (False, "points")
    assert _model_verdict(sb, oracle, proof, values=other_values) == (False, "values")


# ------------------------------------------------------------------------------------------------ 4. the emulated kernels
def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _flat(triples):
    return np.array([v for z in triples for v in z], dtype=np.uint64)


@pytest.mark.parametrize("n", cases.EVAL_LENGTHS)
def test_emulated_evaluation_is_the_models(emu, n):
    coeffs, points, reference = cases.eval_case(n)
    data = np.ascontiguousarray(coeffs)
    for batch, k in cases.eval_shapes(n):
        out = np.full(3 * batch * k, 0xA5A5A5A5, dtype=np.uint64)
        pts = _flat(points[:k])
        assert emu.emu_deep_eval(_ptr(data), n, data.shape[1], batch, _ptr(pts), k, _ptr(out)) == 0
        got = [[tuple(int(v) for v in out[(b * k + j) * 3:(b * k + j) * 3 + 3]) for j in range(k)] for b in range(batch)]
        assert got == [[reference[b][j] for j in range(k)] for b in range(batch)], (n, batch, k)


def test_emulated_evaluation_with_a_stride(emu):
    coeffs, points, reference = cases.eval_case(65, 80)
    data = np.ascontiguousarray(coeffs)
    out = np.zeros(3 * 3 * 2, dtype=np.uint64)
    assert emu.emu_deep_eval(_ptr(data), 65, 80, 3, _ptr(_flat(points[:2])), 2, _ptr(out)) == 0
    assert [tuple(int(v) for v in out[3 * i:3 * i + 3]) for i in range(6)] == [reference[b][j] for b in range(3) for j in range(2)]


def emulated_quotient(emu, case, N, k, out_stride=None):
    out_stride = N if out_stride is None else out_stride
    columns = [np.ascontiguousarray(c) for c in case["columns"]]
    m = len(columns)
    pointers = (ctypes.c_void_p * m)(*[c.ctypes.data for c in columns])
    is_ext = (ctypes.c_int * m)(*[int(c.ndim == 2) for c in columns])
    out = np.full((3, out_stride), 0xA5A5A5A5, dtype=np.uint64)
    rc = emu.emu_deep_quotient(pointers, is_ext, m, case["stride"], N.bit_length() - 1, cases.OFFSET, case["omega"], _ptr(_flat(case["points"])),
                               _ptr(_flat(case["values"])), k, _ptr(np.array(case["lam"], dtype=np.uint64)), _ptr(out), out_stride)
    assert rc == 0
    return out


@pytest.mark.parametrize("N", cases.QUOTIENT_SIZES)
@pytest.mark.parametrize("layout", sorted(cases.LAYOUTS))
@pytest.mark.parametrize("k", cases.POINT_COUNTS)
def test_emulated_quotient_is_the_models(emu, N, layout, k):
    case = cases.quotient_case(N, layout, k)
    assert np.array_equal(emulated_quotient(emu, case, N, k), case["g"])


def test_emulated_quotient_with_strides(emu):
    case = cases.quotient_case(64, "mixed", 2, stride=96)
    out = emulated_quotient(emu, case, 64, 2, out_stride=80)
    assert np.array_equal(out[:, :64], case["g"]) and np.all(out[:, 64:] == 0xA5A5A5A5)


# ------------------------------------------------------------------------------------------------ 5. the domain check
def test_points_of_the_domain_are_refused_before_any_gpu_work(sb):
    N = 64
    pc = sb.PolynomialCommitment(_fri(sb, N, "default"))
    xf = pc.xfield
    omega = xf.modulus.coefficients[0].field.primitive_nth_root(N).value
    inside = [cases.OFFSET, cases.OFFSET * pow(omega, 5, P) % P, cases.OFFSET * pow(omega, N - 1, P) % P]
    for v in inside:
        with pytest.raises(ValueError):
            pc.open(None, [xf.from_limbs([v, 0, 0])], sb.ProofStream())          # (no commitment, no library call: refused first)
        assert pc.in_domain(xf.from_limbs([v, 0, 0])) is True
        assert model.in_domain((v, 0, 0), N, cases.OFFSET)
    with pytest.raises(ValueError):
        pc.open(None, [xf.from_limbs([1, 2, 3]), xf.from_limbs([inside[1], 0, 0])], sb.ProofStream())
    outside = [xf.from_limbs([cases.OFFSET, 1, 0]), xf.from_limbs([cases.OFFSET, 0, 1]), xf.from_limbs([0, 0, 0]), xf.from_limbs([1, 0, 0]),
               xf.from_limbs([cases.OUTSIDE, 0, 0]), xf.from_limbs([cases.OFFSET * omega % P * 3 % P, 0, 0])]
    assert [pc.in_domain(z) for z in outside] == [False] * len(outside)
    assert [model.in_domain(tuple(z.limbs()), N, cases.OFFSET) for z in outside] == [False] * len(outside)


def test_the_new_names_are_public(sb):
    assert sb.PolynomialCommitment is not None and callable(sb.evaluate_at)
    assert "PolynomialCommitment" in sb.__all__ and "evaluate_at" in sb.__all__
    doc = sb.PolynomialCommitment.__doc__
    assert "not hiding" in doc and "AFTER the commitment's root" in doc
