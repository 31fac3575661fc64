"""Openings across commitments on the MI355X: the entry of include/bfstark_rounds.h against the CPython model
(tests/pcs_rounds_model.py), its launch counts against the restated split rule, what it leaves alone (tests/painted.py), the stream it
keeps to (tests/pcs_rounds_stream_child.py), its exports, and PolynomialCommitment.open_rounds / verify_rounds end to end: proof bytes
equal to the model's, both verifiers, and a two-round protocol whose second commitment depends on a challenge drawn behind the first.
Exact integer arithmetic: every comparison is for equality."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import pcs_groups_cases as gcases
import pcs_model as model
import pcs_rounds_cases as cases
import pcs_rounds_model as rmodel
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


# ------------------------------------------------------------------------------------------------ 1. the quotient
def _call(case, buffers, out_ptr, out_stride, launches, stream, entry="rounds"):
    """the argument list of bfsr_deep_quotient_rounds (of bfsx_deep_quotient_groups: no launch count) for a case whose columns lie in `buffers`"""
    from stark_brainfuck_amd import _lib
    args = cases.kernel_arguments(case)
    cols = (_lib.RowColumn * len(args["order"]))()
    for at, c in enumerate(args["order"]):
        cols[at].d_values, cols[at].is_ext, cols[at].field_id = buffers[c].ptr, int(case["columns"][c].ndim == 2), 1
    groups, pairs = len(args["group_columns"]), len(args["pair_point"])
    return [cols, len(args["order"]), case["stride"], case["N"].bit_length() - 1, cases.OFFSET, case["omega"], (u32 * groups)(*args["group_columns"]),
            (u32 * groups)(*args["group_pairs"]), groups, _flat(args["points"]), len(args["points"]), (u32 * pairs)(*args["pair_point"]),
            _flat(args["pair_values"]), (u64 * 3)(*case["lam"]), out_ptr, out_stride] + ([launches] if entry == "rounds" else []) + [stream]


def _quotient(lib, case, out_stride, prefill=None):
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import current_stream
    buffers = [_upload(c) for c in case["columns"]]
    arena = Arena(batch=3, stride=out_stride, n=case["N"])
    if prefill is not None:
        arena.fill_rows(prefill)
    launches = u32(0xFFFF)
    _lib.check(lib.bfsr_deep_quotient_rounds(*_call(case, buffers, arena.ptr, out_stride, ctypes.byref(launches), current_stream())))
    after = arena.contained([("codeword %d" % p, np.ascontiguousarray(c).reshape(-1), buf.to_numpy()) for p, (buf, c) in enumerate(zip(buffers, case["columns"]))])
    return arena.rows(after), launches.value, buffers


@pytest.mark.parametrize("name,N", cases.ALL, ids=cases.IDS)
def test_the_launches_add_up_to_the_models_quotient(sb, lib, name, N):
    """the output in a painted arena, the inputs read back unchanged; as many launches as the restated rule says"""
    case = cases.case(name, N, stride=N + 24)
    got, launches, _ = _quotient(lib, case, N + 40)
    assert launches == len(case["launches"]) == len(rmodel.launches(case["plan"]))
    assert np.array_equal(got, case["g"])


@pytest.mark.parametrize("N", cases.CASE_SIZES["fits"])
def test_a_plan_that_fits_one_launch_is_bfsx_deep_quotient_groups_bit_for_bit(sb, lib, N):
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import current_stream
    case = cases.case("fits", N, stride=N + 24)
    got, launches, buffers = _quotient(lib, case, N + 40)
    assert launches == 1
    old = Arena(batch=3, stride=N + 40, n=N)
    _lib.check(lib.bfsx_deep_quotient_groups(*_call(case, buffers, old.ptr, N + 40, None, current_stream(), entry="groups")))
    assert np.array_equal(old.rows(old.contained()), got)
    assert np.array_equal(got, gcases.plan_tables(N, stride=N + 24)["g"])


@pytest.mark.parametrize("name", ["by_columns", "by_points", "max"])
def test_the_first_launch_does_not_read_the_output(sb, lib, name):
    """the same plan over garbage of two kinds and over paint: the same quotient, so nothing of d_out's content entered it"""
    N = 512
    case = cases.case(name, N, stride=N + 24)
    garbage = np.arange(3 * N, dtype=np.uint64).reshape(3, N) * np.uint64(0x9E3779B97F4A7C15)
    results = [_quotient(lib, case, N + 40, prefill=fill)[0] for fill in (None, garbage, np.full((3, N), P - 1, dtype=np.uint64))]
    assert len(case["launches"]) > 1
    assert all(np.array_equal(r, case["g"]) for r in results)


def test_refused_arguments_leave_the_arena_alone(sb, lib):
    N = 64
    case = cases.case("by_pairs", N)
    buffers = [_upload(c) for c in case["columns"]]
    arena = Arena(batch=3, stride=N, n=N)
    launches = u32(0xFFFF)
    good = _call(case, buffers, arena.ptr, N, ctypes.byref(launches), None)
    assert [list(good[6]), list(good[7]), good[8], good[10]] == [[2] * 5, [4] * 5, 5, 4]

    def rc(**change):
        args = list(good)
        for at, value in change.items():
            args[int(at[1:])] = value
        return lib.bfsr_deep_quotient_rounds(*args)
    ones = lambda count: (u32 * count)(*[1] * count)
    wide = (_lib_columns(buffers[0], 97), )
    refused = {"no column": rc(a1=0), "97 columns": rc(a0=wide[0], a1=97, a6=(u32 * 4)(32, 32, 32, 1), a7=ones(4), a8=4, a11=(u32 * 4)(0, 0, 0, 0)),
               "a group of 33 columns": rc(a0=wide[0], a1=34, a6=(u32 * 2)(33, 1), a7=ones(2), a8=2, a11=(u32 * 2)(0, 0)),
               "no group": rc(a8=0), "25 groups": rc(a0=wide[0], a1=25, a6=ones(25), a7=ones(25), a8=25, a11=(u32 * 25)(*[0] * 25), a12=_flat([(1, 2, 3)] * 25)),
               "no point": rc(a10=0), "25 points": rc(a10=25, a9=_flat([(1 + i, 2, 3) for i in range(25)])), "log_n 0": rc(a3=0), "log_n 25": rc(a3=25),
               "a short limb stride": rc(a2=N - 1), "a short output stride": rc(a15=N - 1), "offset 0": rc(a4=0),
               "sizes that sum to 9": rc(a6=(u32 * 5)(2, 2, 2, 2, 1)), "sizes that sum to 11": rc(a6=(u32 * 5)(2, 2, 2, 2, 3)),
               "an empty group": rc(a6=(u32 * 5)(2, 0, 4, 2, 2)), "a group without a pair": rc(a7=(u32 * 5)(4, 0, 4, 4, 4)),
               "five pairs in a group": rc(a7=(u32 * 5)(5, 3, 4, 4, 4)),
               "49 pairs": rc(a0=wide[0], a1=13, a6=ones(13), a7=(u32 * 13)(*[4] * 12 + [1]), a8=13, a11=(u32 * 49)(*([0, 1, 2, 3] * 12 + [0])), a12=_flat([(1, 2, 3)] * 49)),
               "a pair index of 4": rc(a11=(u32 * 20)(*([0, 1, 2, 3] * 4 + [0, 1, 2, 4]))), "a point twice in a group": rc(a11=(u32 * 20)(*([0, 1, 2, 3] * 4 + [0, 1, 2, 2]))),
               "an unreduced point": rc(a9=_flat([(P, 0, 0)] * 4)), "an unreduced value": rc(a12=_flat([(1, P, 0)] * 20)), "an unreduced lambda": rc(a13=(u64 * 3)(1, 2, P)),
               "output over a codeword": rc(a14=buffers[9].ptr), "a null column": rc(a0=_lib_columns(None, 10))}
    assert refused == {name: 6 for name in refused}
    assert rc(a5=case["omega"] * case["omega"] % P) == 2          # BFS_ERR_NOT_ROOT
    assert launches.value == 0xFFFF                               # (a refused call does not count launches either)
    arena.contained()                                             # nothing was written: not even the first launch of a plan refused late
    assert rc() == 0 and launches.value == 2
    assert rc(a16=None) == 0                                      # the launch count is optional
    assert np.array_equal(arena.rows(arena.contained()), case["g"])


def _lib_columns(buffer, count):
    from stark_brainfuck_amd import _lib
    cols = (_lib.RowColumn * count)()
    for c in range(count):
        cols[c].d_values, cols[c].is_ext, cols[c].field_id = (buffer.ptr if buffer is not None else None), 0, 1
    return cols


# ------------------------------------------------------------------------------------------------ 2. stream order
def test_the_entry_keeps_to_its_stream(sb):
    """tests/pcs_rounds_stream_child.py, once, in a child process under its own time limit"""
    proc = subprocess.run([sys.executable, os.path.join(HERE, "pcs_rounds_stream_child.py")], capture_output=True, text=True, timeout=CHILD_SECONDS)
    lines = [json.loads(l) for l in proc.stdout.splitlines() if l.startswith("{")]
    for l in lines:
        print(json.dumps(l))
    errors = [l["error"] for l in lines if "error" in l]
    assert proc.returncode == 0 and not errors and lines and lines[-1].get("done"), "the child ended with status %s: %s\n%s" % (
        proc.returncode, errors, proc.stderr[-2000:])
    assert [l["ok"] for l in lines if "control" in l] == [True]
    by_case = {l["case"]: l for l in lines if "case" in l}
    assert sorted(by_case) == ["deep_quotient_rounds"]
    for name, line in by_case.items():
        assert line["kind"] == "enqueues" and line["ok"], "%s: %s" % (name, "\n".join(line["failures"]))


# ------------------------------------------------------------------------------------------------ 3. exports
def test_the_library_exports_what_the_header_declares(sb, lib):
    from stark_brainfuck_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "bfstark_rounds.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bfsr_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("bfsr_")}
    assert declared == exported == set(_lib.rounds_exported_symbols()) == {"bfsr_deep_quotient_rounds"}
    assert all(getattr(lib, name).argtypes for name in declared)
    assert '#include "bfstark_open.h"' in text
    # every stream-taking function of the header is a case of the child above
    taking = set(re.findall(r"\b(bfsr_[a-z0-9_]+)\s*\([^;]*void\*\s*stream\)", text))
    import pcs_rounds_stream_child as child
    assert taking == declared == set(child.rounds_case().entries)
    # the signature table has the header's argument count
    arguments = re.search(r"bfsr_deep_quotient_rounds\s*\(([^;]*)\)\s*;", text).group(1)
    assert len(arguments.split(",")) == len(_lib._ROUNDS_SIGNATURES["bfsr_deep_quotient_rounds"][1]) == 18


# ------------------------------------------------------------------------------------------------ 4. end to end
def _fri(sb, N, mode):
    a, coset, bits = cases.MODES[mode]
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    return sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, cases.EXPANSION, cases.T, XF, folding_factor=a, coset_leaves=coset, grinding_bits=bits)


def _commit_rounds(sb, pc, polys, ps):
    """the package's commitments of the model's polynomials, the interludes pushed in between; the caller's order is not the row's: the
    base polynomials are handed over first"""
    commitments = []
    for r, (ext, base) in enumerate(polys):
        handed = [sb.BaseArray.from_numpy(f) for f in base] + [sb.XArray.from_numpy(f, pc.xfield) for f in ext]
        commitments.append(pc.commit(handed, ps))
        if r < len(polys) - 1:
            ps.push(cases.INTERLUDES[r])
    return commitments


@pytest.mark.parametrize("N,mode", cases.PROTOCOL, ids=cases.PROTOCOL_IDS)
def test_proof_bytes_are_the_models_and_both_verifiers_accept(sb, lib, oracle, N, mode):
    """the default mode at N = 64; folding_factor = 8 with coset leaves and 4 grinding bits at N = 256"""
    import test_pcs_host as host
    proof = cases.model_proof(N, mode)
    a, coset, bits = cases.MODES[mode]
    assert (mode == "coset8") == (bits > 0)
    pc = sb.PolynomialCommitment(_fri(sb, N, mode))
    ps = sb.ProofStream()
    commitments = _commit_rounds(sb, pc, proof["polys"], ps)
    assert [c.root() for c in commitments] == proof["roots"] and [len(c.polys) for c in commitments] == proof["widths"]
    assert [pc.global_column(commitments, r, 0) for r in range(3)] == rmodel.first_columns(proof["widths"])
    assert commitments[0].column_of(0) == 5 and commitments[0].column_of(11) == 0          # (base polynomials were handed over first)
    values = pc.open_rounds(commitments, proof["raw_plan"], ps)
    limbs = [[[tuple(v.limbs()) for v in per_point] for per_point in per_group] for per_group in values]
    assert limbs == proof["values"]
    data = ps.serialize()
    assert data == proof["bytes"]
    back = sb.ProofStream().deserialize(data)
    roots = [back.pull() for _ in range(cases.START)]
    roots = [roots[at] for at in cases.ROOT_AT]
    assert pc.verify_rounds(roots, proof["widths"], proof["raw_plan"], values, back) is True
    assert rmodel.verify(oracle, streams.load(oracle, data), cases.START, roots, proof["widths"], proof["raw_plan"], limbs, N, cases.OFFSET, proof["omega"],
                         cases.T, a, coset, host._fri_verify(sb, N, mode)) == (True, "accepted")


def test_one_commitment_gives_the_quotient_of_open_at_and_its_stream_but_for_the_widths(sb, lib, oracle):
    N, mode = 64, "default"
    proof = cases.model_proof(N, mode, single=True)
    pc = sb.PolynomialCommitment(_fri(sb, N, mode))
    ps, ps_at = sb.ProofStream(), sb.ProofStream()
    committed = _commit_rounds(sb, pc, proof["polys"], ps)[0]
    ps_at.push(committed.root())
    values = pc.open_rounds([committed], proof["raw_plan"], ps)
    assert ps.serialize() == proof["bytes"]
    values_at = pc.open_at(committed, proof["raw_plan"], ps_at)
    as_limbs = lambda vs: [[[tuple(v.limbs()) for v in per_point] for per_point in per_group] for per_group in vs]
    assert as_limbs(values) == as_limbs(values_at) == proof["values"]
    # the streams: the same objects in front of the shape, then the widths in the shape (behind it lambda differs, and all it decides)
    assert ps.objects[0] == ps_at.objects[0]
    assert [tuple(z.limbs()) for z in ps.objects[1]] == [tuple(z.limbs()) for z in ps_at.objects[1]]
    assert ps.objects[2] == ((16,), ps_at.objects[2])
    # the quotient codeword under the same lambda
    plan = pc.plan(proof["raw_plan"], 16)
    launches = u32(0)
    g = pc.quotient_rounds([committed], pc.rounds_plan(proof["raw_plan"], [16]), proof["values"], proof["lam"], launches)
    g_at = pc.quotient_at(committed, plan, proof["values"], proof["lam"])
    assert launches.value == 1 and np.array_equal(g.to_numpy(), g_at.to_numpy()) and np.array_equal(g.to_numpy(), proof["g"])
    back = sb.ProofStream().deserialize(ps.serialize())
    assert pc.verify_rounds([back.pull()], [16], proof["raw_plan"], values, back) is True


# ---- a two-round protocol: the second commitment depends on a challenge drawn behind the first
def _poly_mul(f, g):
    out = [0] * (len(f) + len(g) - 1)
    for i, a in enumerate(f):
        for j, b in enumerate(g):
            out[i + j] = (out[i + j] + a * b) % P
    return out


def _two_round_prover(sb, pc, f0, f1, cheat=None):
    """commit f0 and f1; draw alpha; commit q = f0 f1 + alpha f0 (cheat: for alpha + cheat instead); draw z; open all three at z"""
    d = pc.max_coefficients
    ps = sb.ProofStream()
    first = pc.commit([sb.BaseArray.from_numpy(np.array(f0, dtype=np.uint64)), sb.BaseArray.from_numpy(np.array(f1, dtype=np.uint64))], ps)
    alpha = tuple(pc.xfield.sample(ps.prover_fiat_shamir()).limbs())
    used = alpha if cheat is None else model.xadd(alpha, cheat)
    product = _poly_mul(f0, f1)
    assert len(product) <= d
    q = np.zeros((3, len(product)), dtype=np.uint64)
    for l in range(3):
        for i in range(len(product)):
            q[l, i] = ((product[i] if l == 0 else 0) + used[l] * (f0[i] if i < len(f0) else 0)) % P
    second = pc.commit([sb.XArray.from_numpy(q, pc.xfield)], ps)
    z = pc.xfield.sample(ps.prover_fiat_shamir())
    values = pc.open_rounds([first, second], [([pc.global_column([first, second], 0, 0), pc.global_column([first, second], 0, 1),
                                                 pc.global_column([first, second], 1, 0)], [z])], ps)
    return ps.serialize(), values, second.root()


def _two_round_verifier(sb, pc, data, values, second_root=None):
    """reads the roots where the prover pushed them, re-derives alpha and z from the transcript -> (the opening holds, the relation
    q(z) = f0(z) f1(z) + alpha f0(z) holds); the protocol's verifier accepts when both do"""
    ps = sb.ProofStream().deserialize(data)
    first = ps.pull()
    alpha = tuple(pc.xfield.sample(ps.verifier_fiat_shamir()).limbs())
    second = ps.pull()
    z = pc.xfield.sample(ps.verifier_fiat_shamir())
    opened = pc.verify_rounds([first, second if second_root is None else second_root], [2, 1], [([0, 1, 2], [z])], values, ps)
    y0, y1, yq = (tuple(v.limbs()) for v in values[0][0])
    return opened, yq == model.xadd(model.xmul(y0, y1), model.xmul(alpha, y0))


def test_a_two_round_protocol_whose_second_commitment_depends_on_a_drawn_challenge(sb, lib, oracle, capsys):
    N = 64
    pc = sb.PolynomialCommitment(_fri(sb, N, "default"))
    f0 = [int(v) for v in oracle.felt_array(cases.SEED, 0, 8)]
    f1 = [int(v) for v in oracle.felt_array(cases.SEED, 100, 7)] + [P - 1]
    data, values, _ = _two_round_prover(sb, pc, f0, f1)
    y0, y1, yq = (tuple(v.limbs()) for v in values[0][0])
    z = tuple(sb.ProofStream().deserialize(data).objects[2][0].limbs())
    assert (y0, y1) == (model.evaluate_base(f0, z), model.evaluate_base(f1, z))
    assert _two_round_verifier(sb, pc, data, values) == (True, True)
    # q committed for another alpha: every claimed value is true and the opening holds, but not the relation under the transcript's alpha;
    capsys.readouterr()
    cheat_data, cheat_values, cheat_root = _two_round_prover(sb, pc, f0, f1, cheat=(1, 0, 0))
    assert _two_round_verifier(sb, pc, cheat_data, cheat_values) == (True, False)
    capsys.readouterr()
    # and the honest stream is refused, with one line, by a verifier that holds the root of that other q
    assert _two_round_verifier(sb, pc, data, values, second_root=cheat_root) == (False, True)
    assert capsys.readouterr().out.count("\n") == 1
