"""The column pipeline of bfs_gl_ntt (ntt.hip: ntt_run_columns): a batch of multi-pass transforms run column by column, even columns
on the caller's stream and odd ones on the library's second stream.  By default only batches of 64-128 MiB columns take it;
BFS_NTT_PIPELINE=force sends every full-size out-of-place multi-pass batch that way, which is what lets these cases be small.  The
switch is read once per process, so the cases run in child processes (tests/ntt_pipeline_child.py), one per route, each once; the
tests assert on their lines.  Bit for bit throughout: against the oracle, and the forced route against one launch per pass.
(The full-size check of the default route is bench.py --full's guard and tests/test_gpu_parity.py's 2^24 columns, which now take it.)"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_SECONDS = 240
PIPELINED, SINGLE, STAGED, EXPANSION = "pipelined columns", "single launch", "staged", "expansion"
TRANSFORM_CASES = ["three_pass_b2", "three_pass_b3", "three_pass_b5", "two_pass_b2", "strides", "inverse", "coset_quarter", "in_place"]


def run_child(what, pipeline):
    """-> ({case: line}, {case: [route of each tiled call after the case's marker]})"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    env = dict(os.environ, BFS_NTT_PIPELINE=pipeline, BFS_NTT_PLAN_LOG="1")
    for name in ("BFS_NTT_STREAMING", "BFS_NTT_WS_PROBE", "BFS_NTT_EXPAND"):
        env.pop(name, None)
    proc = subprocess.run([sys.executable, os.path.join(HERE, "ntt_pipeline_child.py"), what], env=env, capture_output=True, text=True, timeout=CHILD_SECONDS)
    lines = [json.loads(l) for l in proc.stdout.splitlines() if l.startswith("{")]
    for l in lines:
        print(json.dumps(l))
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


@pytest.fixture(scope="module")
def forced():
    return run_child("cases", "force")


@pytest.fixture(scope="module")
def single():
    return run_child("cases", "0")


@pytest.fixture(scope="module")
def order():
    return run_child("order", "force")


@pytest.mark.parametrize("name", TRANSFORM_CASES)
def test_forced_route_equals_the_oracle_and_one_launch_per_pass(forced, single, name):
    """2^17 (6 + 5 + 6 bits, the smallest three-pass plan) with 2, 3 and 5 columns -- an odd batch puts unequal numbers of columns on
    the two streams --, 2^13 (two passes), strides wider than the transforms, an inverse transform with n^-1, and the two shapes that
    must NOT take the pipeline: a coset evaluation of n/4 coefficients and a call whose input and output overlap.  Columns: splitmix,
    values next to 0, p and 2^32, all p - 1, alternating 1 / p - 1."""
    (f, f_routes), (s, s_routes) = forced, single
    for line in (f[name], s[name]):
        assert all(line["oracle"]), line
        assert line["gaps_kept"] and line["input_kept"], line
    assert f[name]["sha"] == s[name]["sha"]
    want = {"coset_quarter": None, "in_place": STAGED}.get(name, PIPELINED)
    if want is None:
        assert f_routes[name] in ([SINGLE], [EXPANSION]), f_routes[name]
    else:
        assert f_routes[name] == [want], f_routes[name]
    assert s_routes[name] == ([STAGED] if name == "in_place" else [SINGLE]) or (name == "coset_quarter" and s_routes[name] == [EXPANSION]), s_routes[name]


def test_the_call_keeps_to_the_callers_stream(order):
    """with the caller's stream held (tests/stream_hold.py) nothing of a forced-route call has run on either stream; after the hold a
    copy enqueued on the caller's stream behind the call reads every column finished"""
    lines, routes = order
    l = lines["stream_order"]
    assert routes["order_warm"][0] == PIPELINED and routes["order_held"] == [PIPELINED], (routes["order_warm"][:1], routes["order_held"])
    assert l["warm_ok"], l
    assert l["held_before_read"] and l["held_after_read"], "the backlog ended before the output was read: %r" % (l,)
    assert l["untouched_while_held"], l
    assert l["copy_after_call_sees_all"] and l["flag_at_end"], l


def test_a_captured_call_takes_one_launch_per_pass_and_replays(order):
    lines, routes = order
    l = lines["capture"]
    assert routes["capture_warm"] == [PIPELINED] and routes["capture_capturing"] == [SINGLE], routes
    assert l["eager_ok"] and l["capture_ran_nothing"] and l["replays_ok"] == [True, True], l


def test_two_threads_on_two_streams(order):
    lines, routes = order
    assert lines["threads"]["results"] == [[True] * 6, [True] * 6], lines["threads"]
    assert routes["threads"] == [PIPELINED] * 12, routes["threads"]
