"""BrainfuckStark.prove_deep(zero_knowledge=True) / verify_deep(zero_knowledge=True) on the MI355X, unsegmented and segmented (DESIGN.md,
"Zero-knowledge openings"): proof bytes equal to the committed fixtures; every kept trace polynomial against the trace and the blinding
words recomputed from the random stream on the host; the blinded segments against the composition polynomial; the masking polynomial;
what a test can see of hiding; the refusals; and the two modes without zero-knowledge untouched behind it.  Exact integer arithmetic:
every comparison is for equality.  FRI domains here are 2^6 .. 2^11."""
import json
import os

import numpy as np
import pytest

import soundness_cases
from tools import deep_stark_time as deep
from tools import stark_fri_modes as modes
from tools.stark_fri_modes import mode

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
P = soundness_cases.P
CASES = [(name, m, segmented) for name, m, segmented in deep.ZK_FIXTURES if deep.zk_refusal(name, m, segmented) is None]
IDS = [deep.zk_fixture_file(name, m, segmented)[len("deep_zk_"):-len("_proof.bin")] for name, m, segmented in CASES]
SECURE = mode(security_level=8)          # t = 4: k = 14, m = 5


@pytest.fixture(scope="module")
def sb():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import stark_brainfuck_amd
    return stark_brainfuck_amd


_made = {}


def proved(name, m=None, segmented=False):
    """(stark, proof) of program `name` in the zero-knowledge mode on the seeded randomness with the intermediates kept, made once"""
    key = (name, json.dumps(m, sort_keys=True), segmented)
    if key not in _made:
        _made[key] = deep.prove_deep_seeded(name, m, prepare=lambda s: setattr(s, "keep_intermediates", True), segmented=segmented, zero_knowledge=True)
    return _made[key]


def _golden(file):
    return open(os.path.join(GOLDEN, file), "rb").read()


# ------------------------------------------------------------------------------------------------ 1. end to end
@pytest.mark.parametrize("name,m,segmented", CASES, ids=IDS)
def test_verify_deep_accepts_the_proof_and_the_bytes_are_the_fixtures(sb, name, m, segmented):
    stark, proof = proved(name, m, segmented)
    shape = stark.deep_shape(segmented, True)
    assert shape.n <= 1 << 11 and (shape.fri.folding_factor, shape.fri.coset_leaves, shape.fri.grinding_bits) == (
        m["folding_factor"], m["coset_leaves"], m["grinding_bits"])
    assert deep.make_stark(name, m).verify_deep(proof, segmented=segmented, zero_knowledge=True) is True
    assert proof == _golden(deep.zk_fixture_file(name, m, segmented))
    assert stark._last["plan"].widths == (16, 9, shape.s + 1)


def test_the_segmented_shape_of_the_shortest_io_trace_is_refused(sb):
    program, matrices = deep.claim("io")[0], deep.claim("io")[4]
    with pytest.raises(ValueError, match="19 segments of 14 coefficients"):
        deep.make_stark("io").prove_deep(program, *matrices, segmented=True, zero_knowledge=True)


@pytest.mark.parametrize("segmented", [False, True], ids=["unsegmented", "segmented"])
def test_the_loop_with_four_colinearity_checks(sb, segmented):
    stark, proof = proved("loop", SECURE, segmented)
    shape = stark.deep_shape(segmented, True)
    assert (stark.num_colinearity_checks, shape.k, shape.m) == (4, 14, 5 if segmented else 0)
    assert (shape.S, shape.L, shape.s, shape.L0) == ((512, 64, 9, 59) if segmented else (512, 512, 1, 512))
    assert deep.make_stark("loop", SECURE).verify_deep(proof, segmented=segmented, zero_knowledge=True) is True
    assert deep.make_stark("loop").verify_deep(proof, segmented=segmented, zero_knowledge=True) is False          # another security level
    _check_blinding(stark, "loop", segmented)


# ------------------------------------------------------------------------------------------------ 2. the draws, recomputed on the host
def _values(stream, count):
    """`count` base-field values as the prover samples them from a replaced source: 9 bytes each, big-endian, mod p"""
    data = stream(9 * count)
    return [int.from_bytes(data[9 * i:9 * i + 9], "big") % P for i in range(count)]


def _host_draws(stark, name, shape):
    """every draw of a zero-knowledge proof in order, from the seeded stream: per table the randomizer values and blinding rows of the
    base columns, [C0's salts], the two initials, the same for the extension columns' limb planes, [C1's salts], b, R"""
    stream = modes.Stream(deep.zk_seed_tag(name))
    k, n = shape.k, shape.n
    out = {"base": [], "ext": []}
    for kind, skip in (("base", 24 * n), ("ext", 24 * n)):
        for t in stark.tables:
            w = t.base_width if kind == "base" else t.full_width - t.base_width
            if not (t.height and w):
                out[kind].append(None)
                continue
            randomizers = None
            if t.num_randomizers:
                words = 1 if kind == "base" else 3
                randomizers = [[int.from_bytes(data[8 * l:8 * l + 8], "big") % P for l in range(words)] if kind == "ext" else [int.from_bytes(data, "big") % P]
                               for data in (stream(24) for _ in range(w))]
            planes = w if kind == "base" else 3 * w
            flat = _values(stream, planes * k)
            out[kind].append((randomizers, [flat[b * k:(b + 1) * k] for b in range(planes)]))
        stream(skip)          # the commitment's salts
        if kind == "base":
            stream(2 * 24)          # the permutation arguments' initials
    out["b"] = _values(stream, 3 * (shape.s - 1) * shape.m)
    out["R"] = _values(stream, 3 * shape.L)
    return out


def _at(coefficients, x):
    total = 0
    for c in reversed(coefficients):
        total = (total * x + c) % P
    return total


def _unblinded(stark, name, segmented):
    """per kept trace polynomial (base columns, then the limb planes of the extension columns, in table order): (table, u, r, trace) with
    u = kept - (X^h - 1) r on the host, checked to be the interpolant prove_deep makes without blinding"""
    last, shape = stark._last, stark.deep_shape(segmented, True)
    draws = _host_draws(stark, name, shape)
    omega, k = shape.working_domain.omega.value, shape.k
    found = []
    for kind in ("base", "ext"):
        polys = iter(last[kind + "_polys"])
        for t, mine in zip(stark.tables, draws[kind]):
            w = t.base_width if kind == "base" else t.full_width - t.base_width
            h = t.height
            if mine is None:
                for _ in range(w):
                    assert not next(polys).to_numpy().any(), "a column of a table without rows is not zero"
                continue
            randomizers, rows = mine
            traces = t.base_array() if kind == "base" else t._ext_planes().to_numpy()[:3 * w * h].reshape(3 * w, h)
            for c in range(w):
                f = next(polys)
                assert len(f) == h + k
                kept = [[int(v) for v in f.to_numpy()]] if kind == "base" else [[int(v) for v in plane] for plane in f.to_numpy()]
                for l, coefficients in enumerate(kept):
                    plane = c if kind == "base" else 3 * c + l
                    r, trace = rows[plane], [int(v) for v in traces[plane]]
                    u = list(coefficients)
                    for i in range(k):          # minus (X^h - 1) r
                        u[i] = (u[i] + r[i]) % P
                        u[i + h] = (u[i + h] - r[i]) % P
                    assert not any(u[h + 1:]), "%s %s column %d: more than h + 1 coefficients without the blinding" % (name, t.air.name, plane)
                    # folded mod X^h - 1 the kept polynomial is the trace's interpolant: its values on the subgroup are the trace
                    folded = [0] * h
                    for i, v in enumerate(coefficients):
                        folded[i % h] = (folded[i % h] + v) % P
                    assert [_at(folded, pow(t.omicron.value, i, P)) for i in range(h)] == trace, "%s %s column %d" % (name, t.air.name, plane)
                    if randomizers is None:
                        assert u[h] == 0
                    else:          # the rank-one randomizer is still there: the drawn value at the point omega of the working domain
                        assert _at(u, omega) == randomizers[c][l if kind == "ext" else 0]
                    found.append((t, u, r, trace, coefficients))
    return found, draws


def _check_blinding(stark, name, segmented):
    last, shape = stark._last, stark.deep_shape(segmented, True)
    found, draws = _unblinded(stark, name, segmented)
    assert len(found) == 16 + 27 - sum((t.base_width + 3 * (t.full_width - t.base_width)) for t in stark.tables if not t.height)
    assert {t.height for t, *_ in found} >= {h for h in (t.height for t in stark.tables) if h}
    zero_columns = [(u, kept) for _, u, _, trace, kept in found if not any(trace)]
    assert zero_columns and all(any(kept) and kept != u for u, kept in zero_columns), "an identically-zero column must not open as zero"
    assert all(kept != u for _, u, _, _, kept in found)
    # the device's blinding buffers hold the stream's words
    for kind in ("base", "ext"):
        buffers = iter(last[kind + "_blinding"])
        for mine in draws[kind]:
            if mine is not None:
                flat = [v for row in mine[1] for v in row]
                assert [int(v) for v in next(buffers).to_numpy()[:len(flat)]] == flat
    # the masking polynomial and the blinded segments
    L, S, s, m, L0 = shape.L, shape.S, shape.s, shape.m, shape.L0
    R = last["R"].to_numpy()
    assert R.shape == (3, L) and len(last["R"]) == L and [int(v) for v in R.reshape(-1)] == draws["R"]
    H = [[int(v) for v in plane] for plane in last["h_coefficients"].to_numpy()]
    assert len(H[0]) == S and len(last["segments"]) == s and all(len(f) == L for f in last["segments"])
    segments = [[[int(v) for v in plane] for plane in f.to_numpy()] for f in last["segments"]]
    if m == 0:
        assert s == 1 and segments[0] == H and last["b"] is None and last["blinded_segments"] is None
        return found
    import blind_cases as bc
    assert [int(v) for v in last["b"].to_numpy()[:len(draws["b"])]] == draws["b"]
    b = [[draws["b"][(3 * j + l) * m:(3 * j + l + 1) * m] for l in range(3)] for j in range(s - 1)]
    assert segments == bc.split_blind_model(H, S, L0, s, b, m)
    for l, plane in enumerate(bc.recombined(segments, L0, s)):
        assert plane[:S] == H[l] and not any(plane[S:])
    for j in range(s):
        assert segments[j] != [(H[l][j * L0:(j + 1) * L0] + [0] * L)[:L] for l in range(3)], "segment %d is the plain slice" % j
    return found


@pytest.mark.parametrize("name,m,segmented", CASES, ids=IDS)
def test_the_kept_polynomials_are_the_trace_plus_the_streams_blinding(sb, oracle, name, m, segmented):
    """... and what a test can see of hiding: every opened value of every column of a table with rows -- at z, at z * omicron and on
    every point of the commitment domain, the opened rows among them -- differs from the unblinded polynomial's value there"""
    from stark_brainfuck_amd import air
    from stark_brainfuck_amd.pcs import _combine_planes
    stark, _ = proved(name, m, segmented)
    found = _check_blinding(stark, name, segmented)
    last, shape = stark._last, stark.deep_shape(segmented, True)
    n, offset, omega = shape.n, shape.domain.offset.value, shape.domain.omega.value
    committed = np.concatenate([last["committed_base_codewords"].to_numpy()[:16 * n].reshape(16, n), last["committed_ext_codewords"].to_numpy()[:27 * n].reshape(27, n)])
    planes = iter(range(43))
    at = {}
    for t in stark.tables:          # the plane of every kept polynomial among the 16 + 27 committed ones
        at[t, "base"] = [next(planes) for _ in range(t.base_width)]
    for t in stark.tables:
        at[t, "ext"] = [next(planes) for _ in range(3 * (t.full_width - t.base_width))]
    order = {t: at[t, "base"] + at[t, "ext"] for t in stark.tables}
    per_table = {}          # (found lists every table's base columns first, then every table's limb planes)
    for entry in found:
        per_table.setdefault(entry[0], []).append(entry)
    z = last["z"]
    for t, entries in per_table.items():
        base_entries, ext_entries = entries[:t.base_width], entries[t.base_width:]
        assert len(ext_entries) == 3 * (t.full_width - t.base_width)
        for plane, (_, u, _, _, kept) in zip(order[t], base_entries + ext_entries):
            plain = oracle.fast_coset_evaluate(np.array(u, dtype=np.uint64), offset, omega, n)
            assert np.array_equal(committed[plane], oracle.fast_coset_evaluate(np.array(kept, dtype=np.uint64), offset, omega, n))
            assert (committed[plane] != plain).all(), "a committed word is the unblinded polynomial's"
        group = last["opened"][last["plan"].table_group[stark.tables.index(t)]]
        points = [z] if t.height == 1 else [z, air.xscale(z, t.omicron.value)]
        assert len(group) == len(points)
        for values, point in zip(group, points):
            powers = [air.X1]
            for _ in range(t.height + shape.k):
                powers.append(air.xmul(powers[-1], point))
            # a base-coefficient polynomial at a point of F_p^3 (u has zeros behind its h + 1 coefficients: _unblinded has checked)
            value_at = lambda coefficients: tuple(sum(c * powers[i][l] for i, c in enumerate(coefficients)) % P for l in range(3))
            for c in range(t.base_width):
                _, u, _, _, kept = base_entries[c]
                assert tuple(values[c]) == value_at(kept) != value_at(u)
            for c in range(t.full_width - t.base_width):          # an extension column is its three limb planes' values combined
                mine = ext_entries[3 * c:3 * c + 3]
                combined = lambda which: tuple(_combine_planes([value_at(e[which]) for e in mine]))
                assert tuple(values[t.base_width + c]) == combined(4) != combined(1)


def test_the_debug_switch_checks_the_degree_of_the_blinded_composition(sb, monkeypatch):
    monkeypatch.setenv("BFS_DEBUG", "1")
    for segmented in (False, True):
        assert deep.prove_deep_seeded("two_io", segmented=segmented, zero_knowledge=True)[1] == _golden(deep.zk_fixture_file("two_io", mode(), segmented))


def test_two_proofs_on_the_systems_randomness_share_no_root_and_no_opened_row(sb):
    program, matrices = deep.claim("two_io")[0], deep.claim("two_io")[4]
    for segmented in (False, True):
        seen = []
        for _ in range(2):
            stark = deep.make_stark("two_io")
            proof = stark.prove_deep(program, *matrices, segmented=segmented, zero_knowledge=True)
            assert deep.make_stark("two_io").verify_deep(proof, segmented=segmented, zero_knowledge=True) is True
            objects = deep.objects_of(proof)
            rows = [objects[deep.VALUES_AT + 2 + 2 * r] for r in range(3)]          # t = 1: one row per commitment, each before its (salt, path)
            assert [len(row) for row in rows] == [16, 9, stark.deep_shape(segmented, True).s + 1]
            salts = [objects[deep.VALUES_AT + 3 + 2 * r][0] for r in range(3)]
            assert all(isinstance(salt, bytes) and len(salt) == 24 for salt in salts) and len(set(salts)) == 3
            seen.append({"roots": [objects[0], objects[1], objects[deep.ROOT2_AT]],
                         "rows": [tuple(tuple(e.limbs()) if hasattr(e, "limbs") else e.value for e in row) for row in rows], "salts": salts})
        for key in ("roots", "rows", "salts"):
            assert not set(seen[0][key]) & set(seen[1][key]), key


# ------------------------------------------------------------------------------------------------ 3. refusals
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


@pytest.mark.parametrize("name,m,segmented", CASES, ids=IDS)
def test_false_traces_tampered_proofs_and_the_other_modes_proofs_are_refused(sb, name, m, segmented, capsys):
    """every provable fixture in both modes: a proof of a false trace, the byte-level tamperings, and each of the four (segmented,
    zero_knowledge) verifiers against the other three kinds of proof -- this mode's proof made here, the others' the committed fixtures"""
    stark, proof = proved(name, m, segmented)
    verifier = deep.make_stark(name, m)
    kwargs = {"segmented": segmented, "zero_knowledge": True}
    assert verifier.verify_deep(proof, **kwargs) is True
    false_proof = deep.prove_deep_seeded(name, m, matrices=[_false_processor(name)] + list(deep.claim(name)[4])[1:], **kwargs)[1]
    assert isinstance(false_proof, bytes) and false_proof != proof
    verdicts = {"a false trace": _refused(verifier, false_proof, capsys, **kwargs)}
    flipped = bytearray(proof)
    flipped[len(flipped) // 3] ^= 0x10
    verdicts["a flipped byte"] = _refused(verifier, bytes(flipped), capsys, **kwargs)
    changed = dict(deep.tamperings(proof))
    changed.update(deep.zk_tamperings(proof))
    if segmented:
        changed.update(deep.segment_tamperings(proof))
    for what, data in changed.items():
        verdicts[what] = _refused(verifier, data, capsys, **kwargs)
    # each of the four verifiers refuses the other three kinds of proof (`,.` has no segmented zero-knowledge proof: three kinds)
    kinds = [(seg, zk) for seg in (False, True) for zk in (False, True) if not (zk and deep.zk_refusal(name, m, seg))]
    files = {(False, False): deep.fixture_file(name, m), (True, False): deep.segmented_fixture_file(name, m),
             (False, True): deep.zk_fixture_file(name, m, False), (True, True): deep.zk_fixture_file(name, m, True)}
    proofs = {kind: proof if kind == (segmented, True) else _golden(files[kind]) for kind in kinds}
    for made, data in proofs.items():
        for seg, zk in kinds:
            if (seg, zk) == made:
                assert verifier.verify_deep(data, segmented=seg, zero_knowledge=zk) is True
            else:
                verdicts["a proof of mode %s given to the verifier of mode %s" % (made, (seg, zk))] = _refused(verifier, data, capsys, segmented=seg, zero_knowledge=zk)
    assert verdicts == {what: False for what in verdicts} and len(verdicts) == 9 + (2 if segmented else 0) + len(kinds) * (len(kinds) - 1)


# ------------------------------------------------------------------------------------------------ 4. the other modes untouched
@pytest.mark.parametrize("name", ["plus1", "loop"])
def test_the_modes_without_zero_knowledge_give_their_fixtures_after_a_zero_knowledge_proof(sb, name):
    """one object, one process: the shapes, Fri objects and buffers of the zero-knowledge proofs leave nothing behind; without blinding
    lde_tables keeps its rows of hmax + 1 coefficients, and a commitment that is not hiding its unsalted tree"""
    from stark_brainfuck_amd import randomness
    from stark_brainfuck_amd.merkle import Merkle
    from stark_brainfuck_amd.salted_merkle import SaltedMerkle
    stark = deep.make_stark(name)
    stark.keep_intermediates = True
    program, matrices = deep.claim(name)[0], deep.claim(name)[4]
    for segmented in (False, True):
        with randomness.override(modes.Stream(deep.zk_seed_tag(name))):
            hidden = stark.prove_deep(program, *matrices, segmented=segmented, zero_knowledge=True)
        assert hidden == _golden(deep.zk_fixture_file(name, mode(), segmented))
        assert all(isinstance(c.tree, SaltedMerkle) for c in stark._last["commitments"])
    hmax = max(t.height for t in stark.tables)
    for segmented, file in ((False, deep.fixture_file(name, mode())), (True, deep.segmented_fixture_file(name, mode()))):
        with randomness.override(modes.Stream(deep.seed_tag(name))):
            plain = stark.prove_deep(program, *matrices, segmented=segmented)
        assert plain == _golden(file) and stark.verify_deep(plain, segmented=segmented) is True
        last = stark._last
        assert (last["k"], last["m"], last["L0"], last["base_blinding"], last["ext_blinding"], last["b"], last["R"], last["blinded_segments"]) == (
            0, 0, last["L"], [], [], None, None, None)
        assert all(type(c.tree) is Merkle for c in last["commitments"]) and last["plan"].widths == (16, 9, last["s"])
        assert all(len(f) <= hmax + 1 for f in last["base_polys"] + last["ext_polys"])


def test_lde_tables_without_blinding_and_a_commitment_without_hiding_leave_what_they_left_before(sb):
    """tests/deep_plain_paths.py: the buffers of lde_tables(..., keep_coefficients=True), base and extension, and the stream of
    commit + open, as digests -- against those recorded from the commit before `blinding` and `hiding` existed"""
    import deep_plain_paths
    recorded = json.load(open(os.path.join(GOLDEN, "deep_plain_paths.json")))["digests"]
    assert sorted(recorded) == ["base", "bytes_drawn", "commit_open", "extension"] and recorded["base"]["stride"] == recorded["extension"]["stride"] == 17
    assert deep_plain_paths.compute() == recorded
