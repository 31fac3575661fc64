"""Stream order, the third kind of promise of include/bfstark.h ("every call enqueues its kernels on `stream`", "only enqueue work
unless documented otherwise", "synchronises the stream"): every entry point that takes a stream is called on a stream that is HELD
busy (tests/stream_hold.py) with a decoy in its operands, and on a free stream while the default stream is held.

The C-ABI cases (tests/stream_cases.py) run in one fresh child process (tests/stream_order_child.py) that opens three streams only;
this module starts it once and asserts on its lines.  The Python layer is checked here, under a torch stream of its own with the
default stream held: only the bytes are asserted -- a proof opens more streams than the process has hardware queues, so whether it
finished before the hold ended is printed, not asserted."""
import hashlib
import json
import os
import subprocess
import sys
import time

import pytest

import stream_cases as sc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_SECONDS = 240


@pytest.fixture(scope="module")
def child():
    """the child's JSON lines, by what they are about; it runs once"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    proc = subprocess.run([sys.executable, os.path.join(HERE, "stream_order_child.py")], capture_output=True, text=True, timeout=CHILD_SECONDS)
    lines = [json.loads(l) for l in proc.stdout.splitlines() if l.startswith("{")]
    for l in lines:
        print(json.dumps(l))
    errors = [l["error"] for l in lines if "error" in l]
    assert proc.returncode == 0 and not errors and lines and lines[-1].get("done"), "the child ended with status %s: %s\n%s" % (
        proc.returncode, errors, proc.stderr[-2000:])
    return {"control": {l["control"][0]: l for l in lines if "control" in l}, "case": {l["case"]: l for l in lines if "case" in l},
            "pool": [l for l in lines if "pool" in l]}


def test_control_a_stream_runs_while_the_default_stream_is_held(child):
    assert child["control"]["a"]["ok"], child["control"]["a"]


def test_control_a_call_on_the_wrong_stream_is_seen(child):
    assert child["control"]["b"]["ok"], child["control"]["b"]


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_the_call_keeps_to_its_stream(child, name):
    line = child["case"].get(name)
    assert line is not None, "the child did not run this case"
    assert line["ok"], "\n".join(line["failures"])


def test_a_pooled_block_waits_for_the_stream_it_was_released_on(child):
    assert len(child["pool"]) == 2
    for line in child["pool"]:
        assert line["ok"], "%s: %s" % (line["pool"], line["failures"])


# ------------------------------------------------------------------------------------------------ the Python layer
@pytest.fixture(scope="module")
def held(child):
    """(sb, Hold on a probe stream of its own) -- after the child, so that a child that ended badly starts nothing here"""
    import stark_brainfuck_amd as sb
    from stark_brainfuck_amd import _lib
    from stream_hold import Hold
    lib = _lib.load()
    import ctypes
    probe_stream = ctypes.c_void_p()
    _lib.check(lib.bfs_stream_create(ctypes.byref(probe_stream)))
    hold = Hold(lib, probe_stream)
    hold.warm(None)
    return sb, hold


def _finish(hold, what):
    flag = hold.probe()
    took = 1e3 * (time.perf_counter() - hold.enqueued_at)
    from stark_brainfuck_amd import _lib
    _lib.check(hold.lib.bfs_stream_synchronize(None))
    print("%s: %s the hold on the default stream ended (%.1f ms of backlog, %.1f ms on the host since its first enqueue)" % (
        what, "finished before" if flag == 0 else "was still running when", hold.duration_ms(), took))


def test_ntt_under_a_torch_stream_with_the_default_stream_held(held, oracle):
    import torch
    sb, hold = held
    n = 1 << 12
    w = oracle.primitive_nth_root(n)
    v = oracle.felt_array(sc.SEED + 1, 0, n)
    want = oracle.ntt(w, v)
    with torch.cuda.stream(torch.cuda.Stream()):
        assert (sb.ntt(sb.BaseField.main()(w), sb.BaseArray.from_numpy(v)).to_numpy() == want).all(), "warm run"
        hold.hold(None)
        got = sb.ntt(sb.BaseField.main()(w), sb.BaseArray.from_numpy(v)).to_numpy()
        _finish(hold, "sb.ntt")
    assert (got == want).all()


def test_fri_prove_under_a_torch_stream_with_the_default_stream_held(held, oracle):
    import torch
    import fri_folding_model as folding_model
    sb, hold = held
    N, expansion, t = 1 << 10, 4, 4
    omega = oracle.primitive_nth_root(N)
    cw = folding_model.codeword_of(oracle, sc.SEED + N, N, expansion, sc.OFFSET, omega)
    ref = oracle.fri_prove(cw, sc.OFFSET, omega, expansion, t)
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    fri = sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, expansion, t, XF)
    with torch.cuda.stream(torch.cuda.Stream()):
        fri.prove(sb.XArray.from_numpy(cw), sb.ProofStream())          # warm run
        hold.hold(None)
        ps = sb.ProofStream()
        indices = fri.prove(sb.XArray.from_numpy(cw), ps)
        _finish(hold, "Fri.prove")
    assert indices == ref["indices"]
    assert ps.serialize() == ref["proof_stream"].serialize()


def test_stark_prove_under_a_torch_stream_with_the_default_stream_held(held, monkeypatch):
    import torch
    from stark_brainfuck_amd import brainfuck_stark, salted_merkle, table
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    from stark_brainfuck_amd.vm import VirtualMachine
    from test_gpu_stark import GOLDEN, Stream
    sb, hold = held
    name = "plus1"
    g = json.load(open(os.path.join(GOLDEN, "stark_%s.json" % name)))
    program = VirtualMachine.compile(g["program"])
    running_time, input_symbols, output_symbols = VirtualMachine.run(program, input_data=list(g["input"]))
    matrices = VirtualMachine.simulate(program, input_data=list(input_symbols))
    with torch.cuda.stream(torch.cuda.Stream()):
        stark = BrainfuckStark(running_time, len(matrices[1]), program, input_symbols, output_symbols)
        proofs = []
        for attempt in ("warm run", "held"):
            stream = Stream(name.encode())
            for mod in (brainfuck_stark, salted_merkle, table):
                monkeypatch.setattr(mod, "urandom", stream)
            if attempt == "held":
                hold.hold(None)
            proofs.append(stark.prove(program, *matrices))
            if attempt == "held":
                _finish(hold, "BrainfuckStark.prove")
    for proof in proofs:
        assert len(proof) == g["proof_len"] and hashlib.sha256(proof).hexdigest() == g["proof_sha256"]
    assert proofs[1] == open(os.path.join(GOLDEN, "stark_%s_proof.bin" % name), "rb").read()
