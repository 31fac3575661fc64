"""The prover's pointwise stage checked exactly at FRI domains above the goldens (2^17 to 2^24).  The goldens (test_gpu_stark.py) stop
at 2^16, and verify() recomputes the combination at two rows only; above 2^16 nothing else compared these kernels with an independent
computation.  Every size of tests/pointwise_check.py's checks runs on the codewords the prover left in HBM (keep_intermediates):
  * every word of the base, extension, randomizer, quotient and combination codewords is < p;
  * on ~1100 sampled rows (domain edges, unit-distance wrap-arounds, powers of two, uniform rows) every quotient and the combination
    equal the values recomputed in Python integers from the committed codewords (air.evaluate over the expression graphs);
  * over the whole domain, the degrees: combination and randomizer <= max_degree, extension codewords <= the interpolant degree, each
    quotient <= its own bound (every quotient at 2^17 / 2^18, the two difference quotients at the larger sizes).
That covers air_quotient_kernel, difference_quotient_kernel and combination_kernel (the keep_intermediates path).  The production
path -- bfs_zerofier_inverses + bfs_air_combine + bfs_difference_combine from the native stage driver -- commits to its combination
codeword, so the same proof bytes from the same randomness mean the same codeword: the default prover, the Python stage driver
(native_stages = False) and, from 2^20, ragged row windows must write the proof of the checked run.  At 2^22 the combination and
difference kernels (grid capped at 8192 x 256 = 2^21 points) go around their grid-stride loops twice, at 2^24 eight times."""
import gc

import numpy as np
import pytest

import pointwise_check as pc
from test_gpu_config4 import HELLO_WORLD, _setup
from test_gpu_stark import Stream

pytestmark = pytest.mark.gpu


def _nested(outer):                       # tools/stark_scale.py
    return "+" * outer + "[>" + "+" * outer + "[>++++<-]<-]+++."


ECHO_INPUT = "".join(chr(ord("a") + (7 * k) % 26) for k in range(600)) + "\x00"
PROGRAMS = {      # name: (code, input, log2 of the FRI domain)
    "hello_world": (HELLO_WORLD, "", 17),
    # cells that pass through p - 1 and back to 0 hundreds of times: WRAPPING_PROGRAMS[0] of test_gpu_stark.py, scaled up
    "wrapping": ("[->+<][>]+>[-]" + "+" * 40 + "[>" + "-+" * 12 + "-[>+<+]<-]-++++.----", "", 17),
    # 601 input and 600 output symbols (IO tables of height 1024, unit distance 256, padded: iota^(height - length) != 1)
    "echo": (",[++.,]", ECHO_INPUT, 18),
    "nested32": (_nested(32), "", 20),
    "nested64": (_nested(64), "", 22),
    "nested128": (_nested(128), "", 24),
}


def _shift_tweak(shifts):                 # as in test_gpu_stark.py::test_combination_kernel_without_the_grouped_shift_pattern
    return shifts + (np.arange(len(shifts), dtype=np.uint64) * np.uint64(7)) % np.uint64(5)


def _prove(monkeypatch, name, **attributes):
    """one proof of program `name` from the fixed stream of that name; attributes are set on the prover first"""
    from stark_brainfuck_amd import brainfuck_stark, salted_merkle, table
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    from stark_brainfuck_amd.vm import VirtualMachine
    tag = b"pointwise-" + name.encode()
    code, inputs, log_n = PROGRAMS[name]
    if name == "hello_world":
        stark, program, matrices, _ = _setup(monkeypatch, tag, False)
    else:
        program = VirtualMachine.compile(code)
        running_time, input_symbols, output_symbols = VirtualMachine.run(program, input_data=list(inputs))
        matrices = VirtualMachine.simulate(program, input_data=list(input_symbols))
        stark = BrainfuckStark(running_time, len(matrices[1]), program, input_symbols, output_symbols)
        stream = Stream(tag)
        for mod in (brainfuck_stark, salted_merkle, table):
            monkeypatch.setattr(mod, "urandom", stream)
    assert stark.fri.domain.length == 1 << log_n
    for key, value in attributes.items():
        setattr(stark, key, value)
    return stark, stark.prove(program, *matrices)


def _read_back(stark):
    """host copies of the codewords the stage reads, and the spec of the proof"""
    last, n = stark._last, stark.fri.domain.length
    base = [t.base_codewords.to_numpy().reshape(t.base_width, n) for t in stark.tables]
    ext = [t.ext_codewords.to_numpy().reshape(-1, 3, n) for t in stark.tables]
    spec = pc.PointwiseSpec(stark, last["challenges"], last["terminals"], last["quotient_degree_bounds"], last["weights_seed"],
                            shift_tweak=stark._shift_tweak)
    # the weights the prover drew natively are the reference formula's
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    native = BrainfuckStark._sample_weights(len(spec.weights), last["weights_seed"])
    assert [tuple(int(v) for v in w) for w in native] == spec.weights
    return base, ext, last["randomizer_codeword"].to_numpy(), spec


def _quotients(stark):
    """(quotient index, loader of its (3, n) codeword) in the prover's order, one buffer read at a time"""
    n, q = stark.fri.domain.length, 0
    for buf, count in stark._last["quotient_buffers"]:
        for k in range(count):
            yield q, (lambda buf=buf, k=k: buf.to_numpy(3 * n, offset=3 * k * n).reshape(3, n))
            q += 1


def _check(stark, degrees):
    """all checks of one proof; degrees: "all" quotients, or only the "difference" quotients, or None (the combination's degree is
    skipped too: a shift tweak breaks it on purpose)"""
    base, ext, randomizer, spec = _read_back(stark)
    rows = pc.sample_rows(spec.n, spec.unit_distances(), count=1024, seed=spec.n)
    checker = pc.Checker(spec, base, ext, randomizer, rows)
    failures = checker.inputs(degrees=degrees is not None)
    count = 0
    for q, load in _quotients(stark):
        kind = spec.labels[q][1]
        failures += checker.quotient(q, load(), check_degree=degrees == "all" or (degrees == "difference" and kind == "difference"))
        count += 1
    assert count == len(spec.labels)
    failures += checker.combination(stark._last["combination"].to_numpy(), check_degree=degrees is not None)
    assert not failures, "\n".join("%s: %s" % f for f in failures[:20])
    return checker


def _windows(n):
    """ragged row windows tiling the domain: one point, one from 1, one that ends one short of n / 2, one across n / 2 (= 2^21 at 2^22)"""
    cuts = [0, 1, (1 << 16) + 3, n // 2 - 1, n // 2 + 777, n]
    return [(a, b - a) for a, b in zip(cuts, cuts[1:])]


def _checked_proof(monkeypatch, name, degrees, **attributes):
    """the proof of the checked run (its buffers are handed back before the next proof)"""
    stark, proof = _prove(monkeypatch, name, keep_intermediates=True, **attributes)
    _check(stark, degrees)
    del stark
    gc.collect()
    return proof


@pytest.mark.parametrize("name", list(PROGRAMS))
def test_quotients_and_combination_exact(name, monkeypatch):
    log_n = PROGRAMS[name][2]
    proof = _checked_proof(monkeypatch, name, "all" if log_n <= 18 else "difference")
    assert _prove(monkeypatch, name)[1] == proof, "native stage driver"
    assert _prove(monkeypatch, name, native_stages=False)[1] == proof, "Python stage driver, fused combination"
    if log_n >= 20:
        n = 1 << log_n
        assert _prove(monkeypatch, name, _row_windows=_windows(n))[1] == proof, "row windows"


def test_combination_without_the_grouped_shift_pattern_exact_at_2p20(monkeypatch):
    """air_combine_kernel<TABLE, false> at scale: the degree shifts perturbed term by term (no run of equal shifts), the combination
    checked pointwise (its degree bound no longer holds, on purpose) and the fused kernel's proof equal to the checked one"""
    proof = _checked_proof(monkeypatch, "nested32", None, _shift_tweak=_shift_tweak)
    assert _prove(monkeypatch, "nested32", _shift_tweak=_shift_tweak)[1] == proof, "fused combination"
    assert _prove(monkeypatch, "nested32", _shift_tweak=_shift_tweak, _row_windows=_windows(1 << 20))[1] == proof, "row windows"
    assert _prove(monkeypatch, "nested32")[1] != proof                          # (the tweak did change the combination)


def test_the_checker_catches_faults_in_the_real_buffers(monkeypatch):
    """mutations of HOST copies of the buffers of a 2^17 proof: a word of a quotient changed at a row the pointwise half does not look
    at (degree), a whole quotient times 3 (pointwise), a small word stored as v + p (canonical)"""
    stark, _ = _prove(monkeypatch, "hello_world", keep_intermediates=True)
    base, ext, randomizer, spec = _read_back(stark)
    n = spec.n
    rows = pc.sample_rows(n, spec.unit_distances(), count=1024, seed=n)
    checker = pc.Checker(spec, base, ext, randomizer, rows)
    quotients = dict(_quotients(stark))
    q = spec.labels.index(("ProcessorTable", "transition", 3))
    good = quotients[q]()
    assert checker.quotient(q, good) == []
    unsampled = next(i for i in range(n // 3, n) if i not in set(rows))
    bad = good.copy()
    bad[0, unsampled] = (int(bad[0, unsampled]) + 1) % pc.P
    assert {k for k, _ in checker.quotient(q, bad)} == {"degree"}
    bad = np.stack([pc.oracle.hadamard(plane, np.full(n, 3, dtype=np.uint64)) for plane in good])
    assert {k for k, _ in checker.quotient(q, bad)} == {"pointwise"}
    small = next(k for k in range(len(spec.labels)) if (quotients[k]() < (1 << 32) - 1).any())
    bad = quotients[small]()
    limb, row = [int(v[0]) for v in np.nonzero(bad < (1 << 32) - 1)]
    bad[limb, row] += np.uint64(pc.P)
    assert {k for k, _ in checker.quotient(small, bad)} == {"canonical"}
    comb = stark._last["combination"].to_numpy()
    assert checker.combination(comb) == []
    comb[2, unsampled] = (int(comb[2, unsampled]) + 1) % pc.P
    assert {k for k, _ in checker.combination(comb)} == {"degree"}
