"""What the tests of the verifier's REJECTING side share: the verdict of one verifier route as a value that can be compared, and
tests/golden/soundness.json (gen_soundness_golden.py: what the reference's verify said about altered claims and about proofs of
false traces).  No test lives here."""
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ACCEPTED = ("value", True)
MATRICES = ("processor", "memory", "instruction", "input", "output")
P = (1 << 64) - (1 << 32) + 1


def outcome(stark_args, proof, native):
    """('value', bool) / ('assert', message) / ('error', exception type) of BrainfuckStark(*stark_args).verify(proof) on one of the two
    routes (native: csrc/verifier.cpp; otherwise _verify_stream / Fri.verify in Python).  The verdict is computed inside the `try`;
    callers assert on the returned value, outside it, so that no assertion of theirs can be swallowed."""
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    old = os.environ.get("BFS_NATIVE_VERIFY")
    os.environ["BFS_NATIVE_VERIFY"] = "1" if native else "0"
    try:
        verdict = BrainfuckStark(*stark_args).verify(proof)
        result = ("value", verdict) if verdict is True or verdict is False else ("error", "verify returned %r" % (verdict,))
    except AssertionError as e:
        result = ("assert", str(e))
    except Exception as e:          # noqa: BLE001 -- the reference's verifier raises on some malformed streams: the type is the outcome
        result = ("error", type(e).__name__)
    finally:
        if old is None:
            os.environ.pop("BFS_NATIVE_VERIFY", None)
        else:
            os.environ["BFS_NATIVE_VERIFY"] = old
    return result


def recorded(value):
    """an outcome as soundness.json holds it (true / false / "assert: <message>" / "error: <type>") in the form outcome() returns"""
    if value is True or value is False:
        return ("value", value)
    kind, _, rest = value.partition(": ")
    assert kind in ("assert", "error"), value
    return (kind, rest)


def soundness():
    with open(os.path.join(GOLDEN, "soundness.json")) as f:
        return json.load(f)


def claim_entries():
    """[(proof name, entry)] of the `claims` section, for parametrize"""
    return [(name, entry) for name, entries in sorted(soundness()["claims"].items()) for entry in entries]


def claim_args(entry):
    """the constructor arguments of the claim a `claims` entry describes"""
    from stark_brainfuck_amd.algebra import BaseFieldElement
    from stark_brainfuck_amd.vm import VirtualMachine
    program = [BaseFieldElement(w, VirtualMachine.field) for w in entry["program"]]
    return (entry["running_time"], entry["memory_length"], program, list(entry["input"]), list(entry["output"]))


def recorded_claim(name, tag):
    """the reference's outcome for one altered claim about stark_<name>_proof.bin, or None where the fixture has no such entry"""
    for entry in soundness()["claims"].get(name, []):
        if entry["tag"] == tag:
            return recorded(entry["outcome"])
    return None
