"""bfs_gl_ntt on the planted cases of tests/ntt_planted.py: inputs computed so that operands next to 0, 2^32, 2^63 and p stand in front
of the butterflies of ONE chosen register stage of ONE chosen pass -- every stage of every pass of every tile instance the planner uses
for full-size transforms up to 2^20, forward, inverse with n^-1 and as a coset evaluation.  There the device's carry chains
(gl_add_lazy, gl_sub4, gl_mul_fused, gl_canon, the rule which sums stay unreduced) meet unreduced sums that really are >= p, which the
inputs of tests/test_gpu_parity.py produce in the first butterfly block of the first pass only.  tests/test_ntt_planted_host.py shows
on the host emulation that each input reaches its site and every class of operands there; here the output must equal the oracle's
transform of the same input bit for bit -- so every output word is canonical.

Multi-pass sizes also run in place (passes 0 and 1 through the library's intermediate buffer) and in two child processes, each run
once (tests/ntt_planted_child.py): BFS_NTT_STREAMING=1, the non-temporal instantiations of every tile kernel, and BFS_NTT_PIPELINE=force,
the column pipeline with pass 0's loads-only instantiation."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ntt_planted as planted

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_SECONDS = 240
PIPELINED = "pipelined columns"


@pytest.fixture(scope="module")
def sb():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import stark_brainfuck_amd
    from stark_brainfuck_amd import _lib
    _lib.load()            # raises BackendUnavailable if the HIP library is missing: no fallback
    return stark_brainfuck_amd


@pytest.fixture(scope="module")
def emu():
    return planted.emulation()


@pytest.fixture(scope="module")
def inputs_dir(tmp_path_factory):
    """the multi-pass inputs, kept from the tests that build them for the child processes (which build what they do not find)"""
    d = str(tmp_path_factory.mktemp("ntt_planted"))
    yield d
    shutil.rmtree(d, ignore_errors=True)


def raw_ntt(v, logn, call, batch, in_place=False):
    """straight through the C ABI: bfs_gl_ntt on device buffers, `batch` full-size columns n words apart"""
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer, synchronize
    n = 1 << logn
    din = DeviceBuffer.from_numpy(v)
    dout = din if in_place else DeviceBuffer(n * batch)
    _lib.check(_lib.load().bfs_gl_ntt(din.ptr, n, n, dout.ptr, n, logn, batch, call[0], call[1], call[2], 0))
    synchronize(0)
    return dout.to_numpy()


@pytest.mark.parametrize("case", planted.CASES, ids=planted.CASE_IDS)
def test_planted_case_equals_the_oracle(sb, oracle, emu, inputs_dir, case):
    """the transform of the planted input equals the oracle's, bit for bit; multi-pass sizes also with input and output the same buffer"""
    multi = case.logn in planted.MULTI_PASS
    built = planted.build_case(oracle, case, emu, inputs_dir=inputs_dir if multi else None)
    got = raw_ntt(built.x, case.logn, built.call, case.batch)
    wrong = np.flatnonzero(got != built.want)
    assert wrong.size == 0, "%d words differ, the first at %d: %#x, expected %#x" % (wrong.size, wrong[0], int(got[wrong[0]]), int(built.want[wrong[0]]))
    if multi:
        got = raw_ntt(built.x, case.logn, built.call, case.batch, in_place=True)
        wrong = np.flatnonzero(got != built.want)
        assert wrong.size == 0, "in place: %d words differ, the first at %d: %#x, expected %#x" % (wrong.size, wrong[0], int(got[wrong[0]]), int(built.want[wrong[0]]))


def run_child(what, env_switch, inputs_dir):
    """-> ({name: line}, {name: [route of each tiled call after the name's marker]})"""
    env = dict(os.environ, BFS_NTT_PLAN_LOG="1")
    for name in ("BFS_NTT_STREAMING", "BFS_NTT_PIPELINE", "BFS_NTT_WS_PROBE", "BFS_NTT_EXPAND"):
        env.pop(name, None)
    env.update(env_switch)
    proc = subprocess.run([sys.executable, os.path.join(HERE, "ntt_planted_child.py"), what, inputs_dir], env=env, capture_output=True, text=True,
                          timeout=CHILD_SECONDS)
    lines = [json.loads(l) for l in proc.stdout.splitlines() if l.startswith("{")]
    errors = [l["error"] for l in lines if "error" in l]
    assert proc.returncode == 0 and not errors and lines and lines[-1].get("done"), "the child ended with status %s: %s\n%s" % (
        proc.returncode, errors, proc.stderr[-2000:])
    routes, case = {}, None
    for l in proc.stderr.splitlines():
        if l.startswith("case "):
            case = l[5:].strip()
            routes[case] = []
        elif l.startswith("ntt route: ") and case is not None:
            routes[case].append(l[len("ntt route: "):].strip())
    return {l["case"]: l for l in lines if "case" in l}, routes


def test_non_temporal_instantiations_on_the_planted_cases(sb, inputs_dir):
    """BFS_NTT_STREAMING=1: every data access of every pass non-temporal -- other instantiations of the same tile kernels, which a call
    otherwise takes only above 128 MiB.  Every multi-pass case, one call each, in one child process."""
    lines, routes = run_child("streaming", {"BFS_NTT_STREAMING": "1"}, inputs_dir)
    names = [planted.case_id(c) for c in planted.MULTI_PASS_CASES]
    assert sorted(lines) == sorted(names)
    wrong = [n for n in names if lines[n]["oracle"] != [True]]
    assert not wrong, wrong
    assert all(routes[n] == ["single launch"] for n in names), {n: routes[n] for n in names if routes[n] != ["single launch"]}


def test_column_pipeline_on_the_planted_cases(sb, inputs_dir):
    """BFS_NTT_PIPELINE=force: the planted columns of one size, root and direction -- one per site -- as one batch, column by column on
    two streams, pass 0 with non-temporal loads and ordinary stores (an instantiation no other route takes)"""
    lines, routes = run_child("pipeline", {"BFS_NTT_PIPELINE": "force"}, inputs_dir)
    groups = planted.column_groups()
    assert sorted(lines) == sorted(name for name, _ in groups)
    for name, cases in groups:
        assert lines[name]["columns"] == [planted.case_id(c) for c in cases]
        assert len(cases) >= 2 and routes[name] == [PIPELINED], (name, routes[name])
        wrong = [c for c, ok in zip(lines[name]["columns"], lines[name]["oracle"]) if not ok]
        assert not wrong, wrong
