"""The zero-knowledge mode of prove_deep / verify_deep without a GPU ("Zero-knowledge openings"): the shape arithmetic from
its definitions, the opening plan with the masking polynomial, the refusals, the counting argument behind k = 2 t + 6 and m = t + 1 as
ranks over F_p and F_p^3 by Gaussian elimination on integers, an integer model of the blinded-segment identity with a ragged top, and
verify_deep(zero_knowledge=True) on the committed proofs, their tamperings and the proofs of the other modes."""
import hashlib
import os

import pytest

import blind_cases as bc
from tools import deep_stark_time as deep
from tools.stark_fri_modes import mode

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
P = bc.P
MAX_EXT_COLUMNS = 16


def _stark(running_time, memory_rows, program_length, security_level):
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    from stark_brainfuck_amd.vm import VirtualMachine
    program = VirtualMachine.compile("++[>+<-]>.")[:program_length]
    assert len(program) == program_length
    return BrainfuckStark(running_time, memory_rows, program, [], [], 2, security_level)


def _npo2(v):
    return 1 if v <= 1 else 1 << (v - 1).bit_length()


# ------------------------------------------------------------------------------------------------ 1. the shape
# (claim, t) -> S, L, s', N' at expansion factor 4, as the issue's table has them
SHAPES = [((2, 2, 10), 1, 256, 32, 9, 128), ((2, 2, 10), 4, 256, 32, 10, 128), ((2, 2, 10), 16, 512, 64, 11, 256),
          ((1000, 600, 10), 1, 16384, 2048, 9, 8192), ((37254, 37254, 10), 1, 1 << 20, 1 << 17, 9, 1 << 19),
          ((37254, 111546, 10), 1, 1 << 20, 1 << 18, 5, 1 << 20)]


@pytest.mark.parametrize("claim,t,S,L,s,n", SHAPES)
def test_the_shape_follows_from_its_definitions(claim, t, S, L, s, n, monkeypatch):
    from stark_brainfuck_amd import air
    stark = _stark(*claim, security_level=2 * t)
    e = stark.expansion_factor
    assert (e, stark.num_colinearity_checks, stark.fri.num_colinearity_tests) == (4, t, t)
    k, m = 2 * t + 6, t + 1
    # the constructor's analysis (max_transition_degree under all-ones challenges) with h + k - 1 in the place of interpolant_degree()
    bound = 1
    for table in stark.tables:
        if table.height:
            monkeypatch.setattr(table, "interpolant_degree", lambda h=table.height: h + k - 1)
        bound = max(bound, table.max_transition_degree([air.X1] * 11))
    monkeypatch.undo()
    heights = [table.height for table in stark.tables if table.height]
    assert _npo2(1 + bound) == S and _npo2(max(h + k for h in heights)) == L and -(-S // (L - m)) == s and e * L == n
    shape = stark.deep_shape(segmented=True, zero_knowledge=True)
    assert (shape.S, shape.L, shape.s, shape.n, shape.w) == (S, L, s, n, max(n, S))
    assert (shape.k, shape.m, shape.L0, shape.randomizer, shape.hiding) == (k, m, L - m, True, True)
    assert shape.fri.domain.length == n and shape.working_domain.length == shape.w and shape.domain is shape.fri.domain
    assert shape.fri.num_colinearity_tests == t and s + 1 <= MAX_EXT_COLUMNS
    plain = stark.deep_shape(zero_knowledge=True)          # unsegmented: one segment, no segment blinding
    assert (plain.S, plain.L, plain.s, plain.n, plain.w) == (S, S, 1, e * S, e * S)
    assert (plain.k, plain.m, plain.L0, plain.randomizer, plain.hiding) == (k, 0, S, True, True)
    if claim[0] > 2:          # 10 h + 8 k against 16 h: the composition polynomial is no longer than without blinding
        assert S == stark.max_degree + 1 and plain.fri is stark.fri


@pytest.mark.parametrize("name", list(deep.PROGRAMS))
def test_the_other_modes_keep_their_shape_and_gain_the_neutral_fields(name):
    stark = deep.make_stark(name)
    plain, segmented = stark.deep_shape(), stark.deep_shape(segmented=True)
    S, n = stark.max_degree + 1, stark.fri.domain.length
    assert (plain.L, plain.S, plain.s, plain.n, plain.w) == (S, S, 1, n, n) and n == deep.DOMAINS[name]
    assert plain.fri is stark.fri and plain.domain is stark.fri.domain and plain.working_domain is stark.fri.domain
    L = segmented.L
    assert (segmented.S, segmented.s, segmented.n, segmented.w) == (S, S // L, deep.SEGMENTED_DOMAINS[name], max(4 * L, S)) and 4 * L == segmented.n
    again = stark.deep_segmented_shape()
    assert sorted(vars(again)) == sorted(["L", "S", "s", "n", "w", "fri", "domain", "working_domain", "k", "m", "L0", "randomizer", "hiding"])
    assert segmented.fri is again.fri and segmented.working_domain.length == again.working_domain.length == segmented.w
    for shape in (plain, segmented):
        assert (shape.k, shape.m, shape.L0, shape.randomizer, shape.hiding) == (0, 0, shape.L, False, False)


def test_the_plan_with_a_masking_polynomial():
    from stark_brainfuck_amd.deep_stark import deep_opening_plan
    stark = deep.make_stark("two_io")
    z = (5, 6, 7)
    plain, masked = deep_opening_plan(stark.tables, z, segments=9), deep_opening_plan(stark.tables, z, segments=9, randomizer=True)
    assert plain.widths == (16, 9, 9) and masked.widths == (16, 9, 10)
    assert masked.groups[:-1] == plain.groups[:-1] and masked.h_group == plain.h_group == len(masked.groups) - 1
    assert masked.groups[-1] == (list(range(25, 35)), [z]) and plain.groups[-1] == (list(range(25, 34)), [z])
    assert deep_opening_plan(stark.tables, z, segments=15, randomizer=True).widths == (16, 9, 16)


def test_shapes_and_plans_that_are_refused():
    from stark_brainfuck_amd.deep_stark import deep_opening_plan
    stark = deep.make_stark("io")          # heights 4, 8, 2, 1, 1: S = 256 against L = 16, L0 = 14
    with pytest.raises(ValueError, match="19 segments of 14 coefficients, more than the 15 extension columns"):
        stark.deep_shape(segmented=True, zero_knowledge=True)
    assert stark.deep_shape(zero_knowledge=True).s == 1 and stark.deep_shape(segmented=True).s == 8          # the other three shapes exist
    assert deep.zk_refusal("io", mode(), True) and [deep.zk_refusal(name, m, seg) for name, m, seg in deep.ZK_FIXTURES].count(None) == 9
    with pytest.raises(ValueError, match="1 .. 15 segments"):
        deep_opening_plan(stark.tables, (5, 6, 7), segments=16, randomizer=True)
    with pytest.raises(ValueError, match="1 .. 16 segments"):
        deep_opening_plan(stark.tables, (5, 6, 7), segments=17)
    # (m > L0 cannot come out of deep_shape: L >= h + k > 2 t + 6 > 2 m; bfsz_split_blind refuses it, tests/test_gpu_blind_kernels.py)


# ------------------------------------------------------------------------------------------------ 2. the counting argument
def _rank(rows, add, sub, mul, inv, zero):
    """rank of a matrix over a field given by its operations: Gaussian elimination, exact"""
    rows, rank = [list(r) for r in rows], 0
    for col in range(len(rows[0]) if rows else 0):
        pivot = next((i for i in range(rank, len(rows)) if rows[i][col] != zero), None)
        if pivot is None:
            continue
        rows[rank], rows[pivot] = rows[pivot], rows[rank]
        scale = inv(rows[rank][col])
        rows[rank] = [mul(v, scale) for v in rows[rank]]
        for i in range(len(rows)):
            if i != rank and rows[i][col] != zero:
                f = rows[i][col]
                rows[i] = [sub(a, mul(f, b)) for a, b in zip(rows[i], rows[rank])]
        rank += 1
    return rank


def _base_rank(rows):
    return _rank(rows, lambda a, b: (a + b) % P, lambda a, b: (a - b) % P, lambda a, b: a * b % P, lambda a: pow(a, P - 2, P), 0)


def _powers(z, count):
    from stark_brainfuck_amd import air
    out = [air.X1]
    for _ in range(count - 1):
        out.append(air.xmul(out[-1], z))
    return out


@pytest.mark.parametrize("h", [2, 64])
@pytest.mark.parametrize("t", [1, 4])
def test_one_proof_sees_2t_plus_6_independent_functionals_of_a_blinding_polynomial(t, h):
    """what a proof shows of r in f + (X^h - 1) r, r with base-field coefficients: r(x_i) in the t opened rows, r(omicron x_i) through H
    in the same rows, and r(z), r(omicron z) in F_p^3 -- three base-field functionals each.  On k = 2 t + 6 coefficients they have rank
    k (every view has exactly one preimage: uniform); on k - 1 coefficients only k - 1 of the 2 t + 6 are independent"""
    from stark_brainfuck_amd import air
    from stark_brainfuck_amd.algebra import BaseField
    f = BaseField.main()
    n = 4 * _npo2(h + 2 * t + 6)
    omega, offset, omicron = f.primitive_nth_root(n).value, f.generator().value, f.primitive_nth_root(h).value
    indices = [int.from_bytes(hashlib.blake2b(b"zk-rank" + bytes([t, h, i])).digest(), "big") % n for i in range(t)]
    assert len(set(indices)) == t
    xs = [offset * pow(omega, i, P) % P for i in indices]
    z = tuple(int.from_bytes(hashlib.blake2b(b"zk-point" + bytes([t, h, l])).digest()[:8], "big") % P for l in range(3))
    assert z[1] or z[2]
    for k, want in ((2 * t + 6, 2 * t + 6), (2 * t + 5, 2 * t + 5)):
        rows = [[pow(x, j, P) for j in range(k)] for x in xs] + [[pow(x * omicron % P, j, P) for j in range(k)] for x in xs]
        for point in (z, air.xscale(z, omicron)):
            powers = _powers(point, k)
            rows += [[powers[j][l] for j in range(k)] for l in range(3)]
        assert len(rows) == 2 * t + 6 and _base_rank(rows) == want


@pytest.mark.parametrize("t", [1, 4])
def test_a_segment_is_seen_at_t_plus_1_independent_points(t):
    """b_j over F_p^3 with m = t + 1 coefficients against the t opened rows and z: rank m; with m - 1 coefficients rank m - 1 < t + 1"""
    from stark_brainfuck_amd import air
    xs = [(int.from_bytes(hashlib.blake2b(b"zk-seg" + bytes([t, i])).digest()[:8], "big") % P, 0, 0) for i in range(t)]
    z = (3, 1, 4)
    for m, want in ((t + 1, t + 1), (t, t)):
        rows = [_powers(point, m) for point in xs + [z]]
        assert _rank(rows, air.xadd, air.xsub, air.xmul, air.xinv, air.X0) == want


@pytest.mark.parametrize("S,L0,m,s", [(8, 3, 2, 3), (512, 47, 17, 11), (100, 30, 2, 4)])
def test_the_blinded_segments_sum_to_the_polynomial(S, L0, m, s):
    """the integer model of bfsz_split_blind: a ragged top piece (s L0 > S), every piece at most L0 + m coefficients, the sum exact,
    and the verifier's Horner rule in z^L0 on the pieces' values"""
    assert s == -(-S // L0) and s * L0 > S
    H, b = bc.split_operands(S, L0, m, s, seed=S)
    out = bc.split_blind_model(H, S, L0, s, b, m)
    assert all(len(plane) == L0 + m for segment in out for plane in segment) and not any(out[-1][l][L0:] != [0] * m for l in range(3))
    for l, plane in enumerate(bc.recombined(out, L0, s)):
        assert plane[:S] == [v % P for v in H[l]] and not any(plane[S:])
    x = 0x1234567
    for l in range(3):
        at = lambda coefficients: sum(c * pow(x, i, P) for i, c in enumerate(coefficients)) % P
        horner = 0
        for segment in reversed(out):
            horner = (horner * pow(x, L0, P) + at(segment[l])) % P
        assert horner == at(H[l])


# ------------------------------------------------------------------------------------------------ 3. the verifier on the committed proofs
def _golden(file):
    return open(os.path.join(GOLDEN, file), "rb").read()


def _refused(stark, proof, capsys, **kwargs):
    capsys.readouterr()
    verdict = stark.verify_deep(proof, **kwargs)
    printed = capsys.readouterr().out
    assert printed.count("\n") == 1, "a refusal prints one line: %r" % printed
    return verdict, printed


ENTRIES = deep.fixtures(listing=deep.ZK_FIXTURE_LIST)


def test_the_listing_names_every_fixture_once():
    assert [(e["name"], e["args"], e["segmented"]) for e in ENTRIES] == [(name, m, segmented) for name, m, segmented in deep.ZK_FIXTURES]
    proofs = [e for e in ENTRIES if e["file"]]
    assert len(proofs) == 9 and [(e["name"], e["segmented"]) for e in ENTRIES if not e["file"]] == [("io", True)]
    for e in proofs:
        assert e["file"] == deep.zk_fixture_file(e["name"], e["args"], e["segmented"])
        data = _golden(e["file"])
        assert len(data) == e["proof_len"] < (1 << 20) and hashlib.sha256(data).hexdigest() == e["proof_sha256"]
    for e in ENTRIES:
        if not e["file"]:
            assert e["refused"] == deep.zk_refusal(e["name"], e["args"], e["segmented"])


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e["file"]], ids=lambda e: e["file"][len("deep_zk_"):-len("_proof.bin")])
def test_verify_deep_accepts_the_committed_proof_and_refuses_what_was_changed(entry, capsys):
    name, m, segmented = entry["name"], entry["args"], entry["segmented"]
    verifier, proof = deep.make_stark(name, m), _golden(entry["file"])
    shape = verifier.deep_shape(segmented, True)
    assert (shape.n, shape.w, shape.s, shape.L, shape.S, shape.k, shape.m) == tuple(entry[key] for key in (
        "fri_domain_length", "working_domain_length", "segments", "segment_length", "composition_coefficients", "trace_blinding_coefficients",
        "segment_blinding_coefficients")) and shape.n <= 1 << 11
    assert verifier.verify_deep(proof, segmented=segmented, zero_knowledge=True) is True
    changed = dict(deep.tamperings(proof))
    changed.update(deep.zk_tamperings(proof))
    if segmented:
        changed.update(deep.segment_tamperings(proof))
    lines = {}
    for what, data in changed.items():
        verdict, lines[what] = _refused(verifier, data, capsys, segmented=segmented, zero_knowledge=True)
        assert verdict is False, what
    assert lines["a salt of 23 bytes"] == "opened row is not well formed\n"
    assert lines["a flipped salt byte"] == "merkle authentication path verification fails for an opened row\n"
    assert verifier.verify_deep(proof, segmented=segmented, zero_knowledge=True) is True


@pytest.mark.parametrize("name", ["plus1", "two_io", "loop"])
def test_each_of_the_four_verifiers_refuses_the_other_three_proofs(name, capsys):
    verifier = deep.make_stark(name)
    kinds = {(False, False): deep.fixture_file(name, mode()), (True, False): deep.segmented_fixture_file(name, mode()),
             (False, True): deep.zk_fixture_file(name, mode(), False), (True, True): deep.zk_fixture_file(name, mode(), True)}
    for (segmented, zero_knowledge), file in kinds.items():
        proof = _golden(file)
        for seg in (False, True):
            for zk in (False, True):
                if (seg, zk) == (segmented, zero_knowledge):
                    assert verifier.verify_deep(proof, segmented=seg, zero_knowledge=zk) is True
                else:
                    assert _refused(verifier, proof, capsys, segmented=seg, zero_knowledge=zk)[0] is False, (file, seg, zk)
