"""BrainfuckStark.prove_deep / verify_deep: the committed fixtures of the mode, and its time and proof size beside prove().

    python tools/deep_stark_time.py [--program big|loop|...] [--reps 5] [--kernel-reps 20] [--json FILE]
    python tools/deep_stark_time.py --sizes
    python tools/deep_stark_time.py --write-golden DIR
    python tools/deep_stark_time.py --segmented [--program ...] [--reps 5] [--kernel-reps 20] [--json FILE]
    python tools/deep_stark_time.py --write-golden-segmented DIR
    python tools/deep_stark_time.py --zero-knowledge [--program ...] [--reps 5] [--json FILE]
    python tools/deep_stark_time.py --write-golden-zk DIR
    python tools/deep_stark_time.py --secret-input [--program sum2|big|...] [--reps 5] [--json FILE]
    python tools/deep_stark_time.py --write-golden-secret DIR

--secret-input: prove_deep(zero_knowledge=True) on the claim with its input public beside prove_deep(zero_knowledge=True,
secret_input=True) on the claim without it, unsegmented and segmented, alternating in one process by stage, proof bytes and verify_deep of
each (profiles/deep_stark_secret_input.md).  --write-golden-secret DIR writes the secret-input proofs of SECRET_FIXTURES on the seeds
b"deep-zk-secret-" + name, and DIR/deep_zk_secret.json.

--zero-knowledge: prove_deep in its four modes (segmented or not, zero_knowledge or not) alternating in one process by stage, per stage
the cost of zero-knowledge over its twin, proof bytes of all four for the program and the four fixture programs
(profiles/deep_stark_zk.md).  --write-golden-zk DIR writes the zero-knowledge proofs of FIXTURES, unsegmented and segmented, on the seeds
b"deep-zk-" + name, and DIR/deep_zk.json.

--segmented: prove_deep and prove_deep(segmented=True) alternating in one process by stage, proof bytes of both modes for the program and
the four fixture programs, and bfsg_decimate_rows on 2^20 -> 2^19 words over 16 and 27 rows beside a second transform of the kept
coefficients and a device copy of the output bytes (profiles/deep_stark_segmented.md).  --write-golden-segmented DIR writes the segmented
proofs of FIXTURES and DIR/deep_segmented.json, on the same seeds.

Without an option: on the 37 254-cycle program of bench.py --full (FRI domain 2^22) prove_deep and prove (Python stages, stage_timing) by
stage, proof bytes of both, verify_deep, and every bfsc_air_compose launch at log_step 0 and 2 against bfs_air_combine on the same table
with all column weights and every second weight zero (the same sum with more work), alternating in one process on the codewords a proof
left in HBM.  Every figure is a median with min and max; stages from a host clock around work that ends in a stream synchronise, kernels from
device events.  --sizes prints the proof bytes of both modes for the four fixture programs.

--write-golden DIR writes the proofs of FIXTURES on seeded randomness (randomness.override with the SHAKE-256 stream of
tools/stark_fri_modes.py, tag b"deep-" + name) and DIR/deep_stark.json.  The proofs need a GPU; the claims, the seeds and the byte-level
tamperings the tests share with this tool are importable without one.
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import stark_fri_modes as modes          # noqa: E402
from tools.stark_fri_modes import mode              # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE_LIST = "deep_stark.json"
# name -> (source, input): FRI domains 2^8 .. 2^11; both I/O tables empty, of height 1, of height 2, input empty and output of height 1
PROGRAMS = {"plus1": ("+", ""), "io": (",.", "a"), "two_io": (",.,.", "ab"), "loop": ("++[>+<-]>.", "")}
DOMAINS = {"plus1": 1 << 8, "io": 1 << 9, "two_io": 1 << 10, "loop": 1 << 11}
HEIGHTS = {"plus1": (0, 0), "io": (1, 1), "two_io": (2, 2), "loop": (0, 1)}          # input and output table
MODE_A8C_G4 = mode(8, True, 4, security_level=6)
FIXTURES = [(name, mode()) for name in PROGRAMS] + [("two_io", MODE_A8C_G4)]


def fixture_file(name, m):
    return "deep_%s_proof.bin" % name if m == mode() else "deep_%s_%s_proof.bin" % (name, modes.mode_id(m).split("_e")[0])


# the segmented mode (prove_deep(segmented=True)): the same claims, seeds and FRI modes, a list and file names of their own
SEGMENTED_FIXTURE_LIST = "deep_segmented.json"
SEGMENTED_DOMAINS = {"plus1": 1 << 5, "io": 1 << 6, "two_io": 1 << 7, "loop": 1 << 8}          # expansion_factor * L


def segmented_fixture_file(name, m):
    return "deep_segmented_" + fixture_file(name, m)[len("deep_"):]


_claims = {}


def claim(name):
    """(program, running_time, input symbols, output symbols, trace matrices)"""
    from stark_brainfuck_amd.vm import VirtualMachine
    if name not in _claims:
        source, given = PROGRAMS[name] if name in PROGRAMS else (name, "")
        program = VirtualMachine.compile(source)
        running_time, inputs, outputs = VirtualMachine.run(program, input_data=list(given))
        _claims[name] = (program, running_time, inputs, outputs, VirtualMachine.simulate(program, input_data=list(inputs)))
    return _claims[name]


def make_stark(name, m=None, output_symbols=None):
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    m = mode() if m is None else m
    program, running_time, inputs, outputs, matrices = claim(name)
    return BrainfuckStark(running_time, len(matrices[1]), program, inputs, outputs if output_symbols is None else output_symbols,
                          m["log_expansion_factor"], m["security_level"], m["folding_factor"], m["coset_leaves"], m["grinding_bits"])


def seed_tag(name):
    return b"deep-" + name.encode()


def prove_deep_seeded(name, m=None, prepare=None, matrices=None, segmented=False, zero_knowledge=False):
    """-> (stark, proof) of program `name` on the seeded randomness (the zero-knowledge mode on a stream of its own, zk_seed_tag);
    prepare(stark) runs before prove_deep; matrices: other traces"""
    from stark_brainfuck_amd import randomness
    stark = make_stark(name, m)
    if prepare is not None:
        prepare(stark)
    kwargs = {"segmented": True} if segmented else {}
    if zero_knowledge:
        kwargs["zero_knowledge"] = True
    with randomness.override(modes.Stream(zk_seed_tag(name) if zero_knowledge else seed_tag(name))):
        proof = stark.prove_deep(claim(name)[0], *(claim(name)[4] if matrices is None else matrices), **kwargs)
    return stark, proof


# the zero-knowledge mode (prove_deep(zero_knowledge=True)), unsegmented and segmented: the same claims and FRI modes, seeds, a list and
# file names of their own
ZK_FIXTURE_LIST = "deep_zk.json"
ZK_FIXTURES = [(name, m, segmented) for segmented in (False, True) for name, m in FIXTURES]


def zk_seed_tag(name):
    return b"deep-zk-" + name.encode()


def zk_fixture_file(name, m, segmented):
    return ("deep_zk_segmented_" if segmented else "deep_zk_") + fixture_file(name, m)[len("deep_"):]


def zk_refusal(name, m, segmented):
    """the ValueError's text if deep_shape refuses the zero-knowledge shape of this fixture (host arithmetic alone), else None"""
    try:
        make_stark(name, m).deep_shape(segmented, True)
    except ValueError as e:
        return str(e)
    return None


def zk_tamperings(proof):
    """name -> bytes: changes to what only a zero-knowledge proof carries -- the salt behind the first opened row, the masking
    polynomial's value at z (the last value of the last group) -- that verify_deep(zero_knowledge=True) must refuse"""
    objects = objects_of(proof)
    salt_at = VALUES_AT + 3          # values, the quotient's root, the first opened row, then its (salt, path)
    salt, path = objects[salt_at]
    assert isinstance(salt, bytes) and len(salt) == 24

    def with_salt(changed):
        return bytes_of(objects[:salt_at] + [(changed, path)] + objects[salt_at + 1:])
    values = [[list(per_point) for per_point in per_group] for per_group in objects[VALUES_AT]]
    values[-1][0][-1] = _bumped(values[-1][0][-1])
    return {"a flipped salt byte": with_salt(bytes([salt[0] ^ 1]) + salt[1:]), "a salt of 23 bytes": with_salt(salt[:23]),
            "the masking polynomial's value": bytes_of(objects[:VALUES_AT] + [values] + objects[VALUES_AT + 1:])}


def write_golden_zk(directory):
    os.makedirs(directory, exist_ok=True)
    entries = []
    for name, m, segmented in ZK_FIXTURES:
        refusal = zk_refusal(name, m, segmented)
        if refusal is not None:          # (a trace this short has more blinded segments than a commitment has columns: there is no such proof)
            entries.append({"file": None, "name": name, "args": m, "segmented": segmented, "refused": refusal})
            print("no proof of %s %s, segmented: %s" % (name, modes.mode_id(m), refusal), flush=True)
            continue
        stark, proof = prove_deep_seeded(name, m, segmented=segmented, zero_knowledge=True)
        shape = stark.deep_shape(segmented, True)
        assert make_stark(name, m).verify_deep(proof, segmented=segmented, zero_knowledge=True) is True, "%s %s does not verify" % (name, modes.mode_id(m))
        assert prove_deep_seeded(name, m, segmented=segmented, zero_knowledge=True)[1] == proof, "two proofs on the same seed differ"
        source, given = PROGRAMS[name]
        entry = {"file": zk_fixture_file(name, m, segmented), "name": name, "program": source, "input": given, "output": "".join(claim(name)[3]),
                 "args": m, "segmented": segmented, "seed": "shake_256(b'bfs-golden-urandom' + %r)" % zk_seed_tag(name),
                 "fri_domain_length": shape.n, "working_domain_length": shape.w, "segments": shape.s, "segment_length": shape.L,
                 "composition_coefficients": shape.S, "trace_blinding_coefficients": shape.k, "segment_blinding_coefficients": shape.m,
                 "proof_len": len(proof), "proof_sha256": hashlib.sha256(proof).hexdigest()}
        with open(os.path.join(directory, entry["file"]), "wb") as f:
            f.write(proof)
        entries.append(entry)
        print("wrote %s  %d bytes  sha256 %s" % (entry["file"], len(proof), entry["proof_sha256"][:16]), flush=True)
    with open(os.path.join(directory, ZK_FIXTURE_LIST), "w") as f:
        json.dump({"made_by": "tools/deep_stark_time.py --write-golden-zk", "proofs": entries,
                   "randomness": "randomness.override(tools.stark_fri_modes.Stream(b'deep-zk-' + name))"}, f, indent=1, sort_keys=True)
        f.write("\n")


# the secret-input mode (prove_deep(zero_knowledge=True, secret_input=True)): claims WITHOUT their input -- the object is made with
# input_symbols "" and the matrices are those of a run on the secret --, seeds, a list and a file name of their own
SECRET_FIXTURE_LIST = "deep_zk_secret.json"
# name -> (source, the secret the fixtures and timings run on): FRI domains 2^9 .. 2^11 (the loop of sum2 runs once per unit of its first symbol)
SECRET_PROGRAMS = {"read2": (",>,<.", "ab"), "sum2": (",>,<[->+<]>.", "\x02\x03"), "plus1": ("+", ""), "two_io": (",.,.", "ab")}
SECRET_FIXTURES = [("two_io", mode(), False)]

_secret_claims = {}


def secret_claim(name, secret=None):
    """(program, running_time, output symbols, trace matrices) of SECRET_PROGRAMS[name] (else PROGRAMS[name], else the source `name`
    itself) run on `secret` (default: the input listed with the program)"""
    from stark_brainfuck_amd.vm import VirtualMachine
    source, given = SECRET_PROGRAMS.get(name) or PROGRAMS.get(name) or (name, "")
    given = given if secret is None else secret
    if (name, given) not in _secret_claims:
        program = VirtualMachine.compile(source)
        running_time, inputs, outputs = VirtualMachine.run(program, input_data=list(given))
        _secret_claims[name, given] = (program, running_time, outputs, VirtualMachine.simulate(program, input_data=list(inputs)))
    return _secret_claims[name, given]


def make_secret_stark(name, m=None, secret=None, program=None, running_time=None, output_symbols=None):
    """the object of the claim "some input makes the program write this output": input_symbols "" -- it never sees the secret.
    program, running_time, output_symbols: another claim's, for the verifiers that must refuse"""
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    m = mode() if m is None else m
    own_program, own_time, outputs, matrices = secret_claim(name, secret)
    return BrainfuckStark(own_time if running_time is None else running_time, len(matrices[1]), own_program if program is None else program, "",
                          outputs if output_symbols is None else output_symbols, m["log_expansion_factor"], m["security_level"],
                          m["folding_factor"], m["coset_leaves"], m["grinding_bits"])


def secret_seed_tag(name):
    return b"deep-zk-secret-" + name.encode()


def secret_fixture_file(name, m, segmented):
    return ("deep_zk_secret_segmented_" if segmented else "deep_zk_secret_") + fixture_file(name, m)[len("deep_"):]


def secret_refusal(name, m, segmented):
    """the ValueError's text if deep_shape refuses the zero-knowledge shape of this claim, else None"""
    try:
        make_secret_stark(name, m).deep_shape(segmented, True)
    except ValueError as e:
        return str(e)
    return None


def prove_secret_seeded(name, m=None, prepare=None, segmented=False, secret=None, secret_input=True, matrices=None):
    """-> (stark, proof) of the secret-input claim `name` on the seeded randomness; secret_input=False: the same object and matrices
    through the zero-knowledge mode alone (which claims the EMPTY input: its verifier refuses the proof when the program read anything)"""
    from stark_brainfuck_amd import randomness
    stark = make_secret_stark(name, m, secret)
    if prepare is not None:
        prepare(stark)
    kwargs = {"segmented": segmented, "zero_knowledge": True}
    if secret_input:
        kwargs["secret_input"] = True
    program, _, _, own = secret_claim(name, secret)
    with randomness.override(modes.Stream(secret_seed_tag(name))):
        proof = stark.prove_deep(program, *(own if matrices is None else matrices), **kwargs)
    return stark, proof


def write_golden_secret(directory):
    os.makedirs(directory, exist_ok=True)
    entries = []
    for name, m, segmented in SECRET_FIXTURES:
        stark, proof = prove_secret_seeded(name, m, segmented=segmented)
        shape = stark.deep_shape(segmented, True)
        kwargs = {"segmented": segmented, "zero_knowledge": True, "secret_input": True}
        assert make_secret_stark(name, m).verify_deep(proof, **kwargs) is True, "%s %s does not verify" % (name, modes.mode_id(m))
        assert prove_secret_seeded(name, m, segmented=segmented)[1] == proof, "two proofs on the same seed differ"
        source, given = SECRET_PROGRAMS[name]
        entry = {"file": secret_fixture_file(name, m, segmented), "name": name, "program": source, "secret": given,
                 "output": "".join(secret_claim(name)[2]), "args": m, "segmented": segmented,
                 "seed": "shake_256(b'bfs-golden-urandom' + %r)" % secret_seed_tag(name), "fri_domain_length": shape.n,
                 "working_domain_length": shape.w, "segments": shape.s, "segment_length": shape.L, "composition_coefficients": shape.S,
                 "trace_blinding_coefficients": shape.k, "segment_blinding_coefficients": shape.m, "proof_len": len(proof),
                 "proof_sha256": hashlib.sha256(proof).hexdigest()}
        with open(os.path.join(directory, entry["file"]), "wb") as f:
            f.write(proof)
        entries.append(entry)
        print("wrote %s  %d bytes  sha256 %s" % (entry["file"], len(proof), entry["proof_sha256"][:16]), flush=True)
    with open(os.path.join(directory, SECRET_FIXTURE_LIST), "w") as f:
        json.dump({"made_by": "tools/deep_stark_time.py --write-golden-secret", "proofs": entries,
                   "randomness": "randomness.override(tools.stark_fri_modes.Stream(b'deep-zk-secret-' + name))"}, f, indent=1, sort_keys=True)
        f.write("\n")


def fixtures(directory=GOLDEN, listing=FIXTURE_LIST):
    path = os.path.join(directory, listing)
    if not os.path.exists(path):
        return []
    with open(path) as f:
        return json.load(f)["proofs"]


# ---- a proof as its objects: root0, root1, five terminals, root2, then open_rounds' points, shape, values, ...
ROOT2_AT, VALUES_AT = 7, 10


def objects_of(proof):
    from stark_brainfuck_amd.ip import ProofStream
    return list(ProofStream().deserialize(proof).objects)


def bytes_of(objects):
    from stark_brainfuck_amd.ip import ProofStream
    ps = ProofStream()
    for obj in objects:
        ps.push(obj)
    return ps.serialize()


def _bumped(element):
    from stark_brainfuck_amd.air import P
    limbs = list(element.limbs())
    limbs[1] = (limbs[1] + 1) % P
    return element.field.from_limbs(limbs)


def tamperings(proof):
    """name -> bytes: the byte-level changes verify_deep must refuse"""
    objects = objects_of(proof)
    values = [[list(per_point) for per_point in per_group] for per_group in objects[VALUES_AT]]
    values[0][0][1] = _bumped(values[0][0][1])
    root2 = bytearray(objects[ROOT2_AT])
    root2[5] ^= 1
    return {"a limb of an opened value": bytes_of(objects[:VALUES_AT] + [values] + objects[VALUES_AT + 1:]),
            "a limb of a terminal": bytes_of(objects[:2] + [_bumped(objects[2])] + objects[3:]),
            "a digest of the composition's root": bytes_of(objects[:ROOT2_AT] + [bytes(root2)] + objects[ROOT2_AT + 1:]),
            "a truncated proof": proof[:len(proof) // 2]}


def _altered(obj):
    """`obj` with its smallest change -- one bit of a digest or salt, one limb or value of an element plus one, an integer plus one, in a
    list or tuple its first item that can be changed -- or None where there is nothing to change (an empty list)"""
    if isinstance(obj, (bytes, bytearray)):
        return bytes(obj[:len(obj) // 2]) + bytes([obj[len(obj) // 2] ^ 1]) + bytes(obj[len(obj) // 2 + 1:]) if len(obj) else None
    if hasattr(obj, "limbs"):
        return _bumped(obj)
    if hasattr(obj, "value"):
        from stark_brainfuck_amd.air import P
        return type(obj)((obj.value + 1) % P, obj.field)
    if isinstance(obj, int) and not isinstance(obj, bool):
        return obj + 1
    if isinstance(obj, (list, tuple)):
        for i, item in enumerate(obj):
            changed = _altered(item)
            if changed is not None:
                return type(obj)(list(obj[:i]) + [changed] + list(obj[i + 1:]))
    return None


def object_tamperings(proof):
    """name -> bytes: per pushed object of the proof the stream with that one object changed (_altered), whatever the stream's layout"""
    objects = objects_of(proof)
    out = {}
    for i, obj in enumerate(objects):
        changed = _altered(obj)
        if changed is not None:
            out["object %d of %d (%s)" % (i, len(objects), type(obj).__name__)] = bytes_of(objects[:i] + [changed] + objects[i + 1:])
    return out


def segment_tamperings(proof):
    """name -> bytes: changes to the opened segment values (the last group of a segmented proof's values) verify_deep must refuse"""
    objects = objects_of(proof)

    def with_segments(change):
        values = [[list(per_point) for per_point in per_group] for per_group in objects[VALUES_AT]]
        values[-1][0] = change(values[-1][0])
        return bytes_of(objects[:VALUES_AT] + [values] + objects[VALUES_AT + 1:])
    segments = list(objects[VALUES_AT][-1][0])
    assert len(segments) >= 2 and segments[0].limbs() != segments[1].limbs()
    return {"a segment value replaced by another canonical value": with_segments(lambda v: v[:-1] + [_bumped(v[-1])]),
            "two segment values swapped": with_segments(lambda v: [v[1], v[0]] + v[2:])}


def write_golden(directory, segmented=False):
    os.makedirs(directory, exist_ok=True)
    entries = []
    option = "--write-golden-segmented" if segmented else "--write-golden"
    for name, m in FIXTURES:
        stark, proof = prove_deep_seeded(name, m, segmented=segmented)
        length = stark.deep_shape(segmented).n
        assert length == (SEGMENTED_DOMAINS if segmented else DOMAINS)[name]
        kwargs = {"segmented": True} if segmented else {}
        assert make_stark(name, m).verify_deep(proof, **kwargs) is True, "%s %s does not verify" % (name, modes.mode_id(m))
        assert prove_deep_seeded(name, m, segmented=segmented)[1] == proof, "two proofs on the same seed differ"
        source, given = PROGRAMS[name]
        entry = {"file": (segmented_fixture_file if segmented else fixture_file)(name, m), "name": name, "program": source, "input": given,
                 "output": "".join(claim(name)[3]), "args": m, "seed": "shake_256(b'bfs-golden-urandom' + %r)" % seed_tag(name),
                 "fri_domain_length": length, "proof_len": len(proof), "proof_sha256": hashlib.sha256(proof).hexdigest()}
        if segmented:
            shape = stark.deep_segmented_shape()
            entry.update({"segments": shape.s, "segment_length": shape.L, "working_domain_length": shape.w})
        with open(os.path.join(directory, entry["file"]), "wb") as f:
            f.write(proof)
        entries.append(entry)
        print("wrote %s  %d bytes  sha256 %s" % (entry["file"], len(proof), entry["proof_sha256"][:16]), flush=True)
    with open(os.path.join(directory, SEGMENTED_FIXTURE_LIST if segmented else FIXTURE_LIST), "w") as f:
        json.dump({"made_by": "tools/deep_stark_time.py " + option, "randomness": "randomness.override(tools.stark_fri_modes.Stream(b'deep-' + name))",
                   "proofs": entries}, f, indent=1, sort_keys=True)
        f.write("\n")


# ---- timing
def _sync():
    from stark_brainfuck_amd.device import current_stream, synchronize
    synchronize(current_stream())


def _mmm(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def sizes():
    """proof bytes of prove and prove_deep for the four fixture programs"""
    rows = []
    for name in PROGRAMS:
        program, _, _, _, matrices = claim(name)
        rows.append({"program": name, "fri_domain_length": DOMAINS[name], "prove_bytes": len(make_stark(name).prove(program, *matrices)),
                     "prove_deep_bytes": len(make_stark(name).prove_deep(program, *matrices))})
        print("SIZE " + json.dumps(rows[-1], sort_keys=True), flush=True)
    return rows


def time_proofs(name, reps):
    """prove_deep and prove (Python stages) by stage, ms; proof bytes; verify_deep"""
    program, _, _, _, matrices = claim(name)
    out = {}
    for label in ("prove_deep", "prove"):
        per_stage, totals, proof = {}, [], None
        for rep in range(reps + 1):
            stark = make_stark(name)
            stark.stage_timing = True
            t0 = time.perf_counter()
            proof = getattr(stark, label)(program, *matrices)
            _sync()
            if rep:          # (the first proof of a shape warms it and is dropped)
                totals.append((time.perf_counter() - t0) * 1e3)
                for stage, seconds in stark.timing.items():
                    per_stage.setdefault(stage, []).append(seconds * 1e3)
        out[label] = {"total_ms": _mmm(totals), "stages_ms": {s: _mmm(v) for s, v in per_stage.items()}, "proof_bytes": len(proof),
                      "fri_domain_length": stark.fri.domain.length}
        out[label + "_proof"] = proof
    verify_ms = []
    for rep in range(reps + 1):
        verifier = make_stark(name)
        t0 = time.perf_counter()
        assert verifier.verify_deep(out["prove_deep_proof"]) is True
        verify_ms.append((time.perf_counter() - t0) * 1e3)
    out["verify_deep_ms"] = _mmm(verify_ms[1:])
    del out["prove_deep_proof"], out["prove_proof"]
    return out


def time_kernels(name, reps):
    """per table with rows: bfsc_air_compose at log_step 0 and 2 and the yardstick bfs_air_combine (column weights and wb zero, zerofier
    inverses computed in the kernel, as the compose kernel computes them), alternating, device events, us"""
    import numpy as np
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.arrays import XArray
    from stark_brainfuck_amd.device import current_stream
    from stark_brainfuck_amd.table import _air_arguments
    lib, stream = _lib.load(), current_stream()
    program, _, _, _, matrices = claim(name)
    stark = make_stark(name)
    stark.keep_intermediates = True          # (the codewords stay in HBM)
    stark.prove_deep(program, *matrices)
    last, domain, n = stark._last, stark.fri.domain, stark.fri.domain.length
    challenges, terminals, weights = last["challenges"], last["terminals"], last["weights"]
    shifts = stark._layout.shifts(stark._quotient_degree_bounds(challenges, terminals))
    start, stop = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(lib.bfs_event_create(ctypes.byref(start)))
    _lib.check(lib.bfs_event_create(ctypes.byref(stop)))

    def timed(call):
        _lib.check(lib.bfs_event_record(start, stream))
        call()
        _lib.check(lib.bfs_event_record(stop, stream))
        _sync()
        ms = ctypes.c_float()
        _lib.check(lib.bfs_event_elapsed_ms(start, stop, ctypes.byref(ms)))
        return ms.value * 1e3
    full, quarter, combined = XArray.empty(n, stark.xfield), XArray.empty(n >> 2, stark.xfield), XArray.empty(n, stark.xfield)
    _lib.check(lib.bfs_memset(combined.ptr, 0, 3 * n * 8, stream))
    rows, at = [], 0
    for k, t in enumerate(stark.tables):
        nq = t.num_quotients()
        mine = np.ascontiguousarray(weights[at:at + nq])
        at += nq
        if not t.height:
            continue
        limbs = mine.reshape(-1).ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        head = (t.table_index, t.base_codewords.ptr, t.ext_codewords.ptr) + tuple(t._domain_arguments(domain)) + tuple(_air_arguments(t, challenges, terminals))
        layout = stark._layout
        terms = np.zeros((t.full_width + nq, 7), dtype=np.uint64)
        terms[:, 6] = shifts[layout.base[k]] + shifts[layout.ext[k]] + shifts[layout.quot[k]]
        terms[t.full_width:, 0:3] = mine
        calls = {"compose_step1": lambda: _lib.check(lib.bfsc_air_compose(*head, limbs, 0, 1, full.ptr, stream)),
                 "compose_step4": lambda: _lib.check(lib.bfsc_air_compose(*head, limbs, 2, 1, quarter.ptr, stream)),
                 "combine_yardstick": lambda: t.combine_into(domain, challenges, terminals, terms, combined)}
        series = {label: [] for label in calls}
        for rep in range(reps + 2):
            for label, call in calls.items():
                us = timed(call)
                if rep >= 2:
                    series[label].append(us)
        row = {"table": t.air.name, "height": t.height, "us": {label: _mmm(v) for label, v in series.items()}}
        base = row["us"]["combine_yardstick"]
        row["allowance_us"] = round(base["median"] + (base["max"] - base["min"]), 4)
        row["within_yardstick"] = row["us"]["compose_step1"]["median"] <= row["allowance_us"]
        row["step4_over_step1"] = round(row["us"]["compose_step4"]["median"] / row["us"]["compose_step1"]["median"], 4)
        rows.append(row)
        print("KERNEL " + json.dumps(row, sort_keys=True), flush=True)
    return rows


def segmented_sizes():
    """proof bytes of prove_deep in both modes for the four fixture programs"""
    rows = []
    for name in PROGRAMS:
        program, _, _, _, matrices = claim(name)
        rows.append({"program": name, "fri_domain_length": DOMAINS[name], "segmented_fri_domain_length": SEGMENTED_DOMAINS[name],
                     "prove_deep_bytes": len(make_stark(name).prove_deep(program, *matrices)),
                     "prove_deep_segmented_bytes": len(make_stark(name).prove_deep(program, *matrices, segmented=True))})
        print("SIZE " + json.dumps(rows[-1], sort_keys=True), flush=True)
    return rows


def time_segmented(name, reps):
    """prove_deep in both modes by stage, ms, ALTERNATING in one process (a warm-up proof of each first, dropped); proof bytes; verify_deep"""
    program, _, _, _, matrices = claim(name)
    legs = {"prove_deep": {}, "prove_deep_segmented": {"segmented": True}}
    series = {label: {"totals": [], "stages": {}} for label in legs}
    proofs, lengths = {}, {}
    for rep in range(reps + 1):
        for label, kwargs in legs.items():
            stark = make_stark(name)
            stark.stage_timing = True
            t0 = time.perf_counter()
            proofs[label] = stark.prove_deep(program, *matrices, **kwargs)
            _sync()
            if rep:
                series[label]["totals"].append((time.perf_counter() - t0) * 1e3)
                for stage, seconds in stark.timing.items():
                    series[label]["stages"].setdefault(stage, []).append(seconds * 1e3)
            lengths[label] = stark.deep_shape(bool(kwargs)).n
    out = {}
    for label, kwargs in legs.items():
        verify_ms = []
        for rep in range(3):
            t0 = time.perf_counter()
            assert make_stark(name).verify_deep(proofs[label], **kwargs) is True
            verify_ms.append((time.perf_counter() - t0) * 1e3)
        out[label] = {"total_ms": _mmm(series[label]["totals"]), "stages_ms": {s: _mmm(v) for s, v in series[label]["stages"].items()},
                      "proof_bytes": len(proofs[label]), "fri_domain_length": lengths[label], "verify_ms": _mmm(verify_ms[1:])}
    out["segmented_median_below_unsegmented_min"] = out["prove_deep_segmented"]["total_ms"]["median"] < out["prove_deep"]["total_ms"]["min"]
    return out


ZK_LEGS = {"prove_deep": {}, "prove_deep_segmented": {"segmented": True}, "prove_deep_zk": {"zero_knowledge": True},
           "prove_deep_segmented_zk": {"segmented": True, "zero_knowledge": True}}


def time_zero_knowledge(name, reps):
    """prove_deep in its four modes by stage, ms, ALTERNATING in one process (a warm-up proof of each first, dropped); proof bytes;
    verify_deep; per stage the median cost of zero-knowledge over the mode's twin without it"""
    program, _, _, _, matrices = claim(name)
    series = {label: {"totals": [], "stages": {}} for label in ZK_LEGS}
    proofs, shapes = {}, {}
    for rep in range(reps + 1):
        for label, kwargs in ZK_LEGS.items():
            stark = make_stark(name)
            stark.stage_timing = True
            t0 = time.perf_counter()
            proofs[label] = stark.prove_deep(program, *matrices, **kwargs)
            _sync()
            if rep:
                series[label]["totals"].append((time.perf_counter() - t0) * 1e3)
                for stage, seconds in stark.timing.items():
                    series[label]["stages"].setdefault(stage, []).append(seconds * 1e3)
            shape = stark.deep_shape(**kwargs)
            shapes[label] = {key: getattr(shape, key) for key in ("L", "S", "s", "n", "w", "k", "m", "L0")}
    out = {}
    for label, kwargs in ZK_LEGS.items():
        verify_ms = []
        for rep in range(3):
            t0 = time.perf_counter()
            assert make_stark(name).verify_deep(proofs[label], **kwargs) is True
            verify_ms.append((time.perf_counter() - t0) * 1e3)
        out[label] = {"total_ms": _mmm(series[label]["totals"]), "stages_ms": {s: _mmm(v) for s, v in series[label]["stages"].items()},
                      "proof_bytes": len(proofs[label]), "shape": shapes[label], "verify_ms": _mmm(verify_ms[1:])}
    for plain in ("prove_deep", "prove_deep_segmented"):
        a, b = out[plain], out[plain + "_zk"]
        out[plain + "_zk"]["cost_over_twin_ms"] = dict({s: round(b["stages_ms"][s]["median"] - a["stages_ms"][s]["median"], 4) for s in a["stages_ms"]},
                                                       total=round(b["total_ms"]["median"] - a["total_ms"]["median"], 4))
    return out


def zero_knowledge_sizes():
    """proof bytes of prove_deep in its four modes for the four fixture programs"""
    rows = []
    for name in PROGRAMS:
        program, _, _, _, matrices = claim(name)
        rows.append(dict({label + "_bytes": None if kwargs.get("zero_knowledge") and zk_refusal(name, mode(), kwargs.get("segmented", False))
                          else len(make_stark(name).prove_deep(program, *matrices, **kwargs)) for label, kwargs in ZK_LEGS.items()}, program=name))
        print("SIZE " + json.dumps(rows[-1], sort_keys=True), flush=True)
    return rows


def time_secret_input(name, reps):
    """the zero-knowledge mode with the claim's input public beside secret_input=True (the object made without the input), unsegmented
    and segmented where the shape exists, by stage, ms, ALTERNATING in one process (a warm-up proof of each first, dropped); proof bytes;
    verify_deep.  name: a key of SECRET_PROGRAMS, or "big" (which reads nothing: the two claims differ in the terminal alone)"""
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    program, running_time, outputs, matrices = secret_claim(name)
    given = (SECRET_PROGRAMS.get(name) or PROGRAMS.get(name) or (name, ""))[1]
    make = {False: lambda: BrainfuckStark(running_time, len(matrices[1]), program, list(given), outputs), True: lambda: make_secret_stark(name)}
    legs = {}
    for segmented in (False, True):
        if secret_refusal(name, mode(), segmented) is None:
            for secret in (False, True):
                label = "prove_deep%s_zk%s" % ("_segmented" if segmented else "", "_secret" if secret else "")
                legs[label] = (secret, dict({"segmented": segmented, "zero_knowledge": True}, **({"secret_input": True} if secret else {})))
    series = {label: {"totals": [], "stages": {}} for label in legs}
    proofs = {}
    for rep in range(reps + 1):
        for label, (secret, kwargs) in legs.items():
            stark = make[secret]()
            stark.stage_timing = True
            t0 = time.perf_counter()
            proofs[label] = stark.prove_deep(program, *matrices, **kwargs)
            _sync()
            if rep:
                series[label]["totals"].append((time.perf_counter() - t0) * 1e3)
                for stage, seconds in stark.timing.items():
                    series[label]["stages"].setdefault(stage, []).append(seconds * 1e3)
    out = {}
    for label, (secret, kwargs) in legs.items():
        verify_ms = []
        for rep in range(3):
            t0 = time.perf_counter()
            assert make[secret]().verify_deep(proofs[label], **kwargs) is True
            verify_ms.append((time.perf_counter() - t0) * 1e3)
        out[label] = {"total_ms": _mmm(series[label]["totals"]), "stages_ms": {s: _mmm(v) for s, v in series[label]["stages"].items()},
                      "proof_bytes": len(proofs[label]), "verify_ms": _mmm(verify_ms[1:])}
    for label in [l for l in legs if l.endswith("_secret")]:
        a, b = out[label[:-len("_secret")]], out[label]
        b["cost_over_twin_ms"] = dict({s: round(b["stages_ms"][s]["median"] - a["stages_ms"][s]["median"], 4) for s in a["stages_ms"]},
                                      total=round(b["total_ms"]["median"] - a["total_ms"]["median"], 4))
        b["bytes_over_twin"] = b["proof_bytes"] - a["proof_bytes"]
    return out


def time_decimation(reps, log_in=20, log_out=19, coefficients=(1 << 16) + 1):
    """bfsg_decimate_rows from 2^log_in to 2^log_out words per row over 16 and 27 rows, beside the alternative it was chosen against -- a
    second transform of the kept `coefficients` coefficients per row onto the 2^log_out points -- and a device copy of the same output
    bytes; alternating, device events, us"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.algebra import BaseField
    from stark_brainfuck_amd.arrays import raw_ntt
    from stark_brainfuck_amd.device import DeviceBuffer, current_stream
    lib, stream, f = _lib.load(), current_stream(), BaseField.main()
    n_in, n_out = 1 << log_in, 1 << log_out
    omega, offset = f.primitive_nth_root(n_out).value, f.generator().value
    start, stop = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(lib.bfs_event_create(ctypes.byref(start)))
    _lib.check(lib.bfs_event_create(ctypes.byref(stop)))

    def timed(call):
        _lib.check(lib.bfs_event_record(start, stream))
        call()
        _lib.check(lib.bfs_event_record(stop, stream))
        _sync()
        ms = ctypes.c_float()
        _lib.check(lib.bfs_event_elapsed_ms(start, stop, ctypes.byref(ms)))
        return ms.value * 1e3
    rows_out = []
    for rows in (16, 27):
        source, coeffs, out = DeviceBuffer(rows * n_in), DeviceBuffer(rows * coefficients), DeviceBuffer(rows * n_out)
        for buf in (source, out):
            _lib.check(lib.bfs_memset(buf.ptr, 1, buf.nbytes, stream))
        _lib.check(lib.bfs_memset(coeffs.ptr, 0, coeffs.nbytes, stream))
        calls = {"decimate": lambda: _lib.check(lib.bfsg_decimate_rows(source.ptr, n_in, log_in - log_out, out.ptr, n_out, n_out, rows, stream)),
                 "second_ntt": lambda: raw_ntt(coeffs.ptr, coefficients, coefficients, out.ptr, n_out, log_out, rows, omega, offset, 1, stream),
                 "device_copy": lambda: _lib.check(lib.bfs_memcpy_d2d(out.ptr, source.ptr, rows * n_out * 8, stream))}
        series = {label: [] for label in calls}
        for rep in range(reps + 2):
            for label, call in calls.items():
                us = timed(call)
                if rep >= 2:
                    series[label].append(us)
        rows_out.append({"rows": rows, "words_in": n_in, "words_out": n_out, "us": {label: _mmm(v) for label, v in series.items()}})
        print("DECIMATE " + json.dumps(rows_out[-1], sort_keys=True), flush=True)
        for buf in (source, coeffs, out):
            buf.free()
    return rows_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--program", default="big")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--sizes", action="store_true")
    ap.add_argument("--segmented", action="store_true", help="both modes of prove_deep alternating, their proof sizes, the decimation kernel")
    ap.add_argument("--write-golden", default=None)
    ap.add_argument("--write-golden-segmented", default=None)
    ap.add_argument("--zero-knowledge", action="store_true", help="the four modes of prove_deep alternating, their proof sizes")
    ap.add_argument("--write-golden-zk", default=None)
    ap.add_argument("--secret-input", action="store_true", help="the zero-knowledge mode with and without secret_input alternating, their proof sizes")
    ap.add_argument("--write-golden-secret", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is proven or timed here")
    if args.write_golden:
        return write_golden(args.write_golden)
    if args.write_golden_segmented:
        return write_golden(args.write_golden_segmented, segmented=True)
    if args.write_golden_zk:
        return write_golden_zk(args.write_golden_zk)
    if args.write_golden_secret:
        return write_golden_secret(args.write_golden_secret)
    result = {}
    if args.secret_input:
        name = args.program
        if name == "big":
            SECRET_PROGRAMS["big"] = (modes.BIG, "")
        result["program"] = name
        result["proofs"] = time_secret_input(name, args.reps)
        print("SECRET_INPUT " + json.dumps(result["proofs"], sort_keys=True), flush=True)
        SECRET_PROGRAMS.pop("big", None)
    elif args.zero_knowledge:
        name = args.program
        if name == "big":
            PROGRAMS["big"] = (modes.BIG, "")
        result["program"] = name
        result["proofs"] = time_zero_knowledge(name, args.reps)
        print("ZERO_KNOWLEDGE " + json.dumps(result["proofs"], sort_keys=True), flush=True)
        PROGRAMS.pop("big", None)
        result["sizes"] = zero_knowledge_sizes()
    elif args.segmented:
        name = args.program
        if name == "big":
            PROGRAMS["big"] = (modes.BIG, "")
        result["program"] = name
        result["proofs"] = time_segmented(name, args.reps)
        print("SEGMENTED " + json.dumps(result["proofs"], sort_keys=True), flush=True)
        PROGRAMS.pop("big", None)
        result["sizes"] = segmented_sizes()
        result["decimation"] = time_decimation(args.kernel_reps)
    elif args.sizes:
        result["sizes"] = sizes()
    else:
        name = args.program
        if name == "big":
            PROGRAMS["big"] = (modes.BIG, "")
        result["program"] = name
        result["proofs"] = time_proofs(name, args.reps)
        print("PROOFS " + json.dumps(result["proofs"], sort_keys=True), flush=True)
        result["kernels"] = time_kernels(name, args.kernel_reps)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
