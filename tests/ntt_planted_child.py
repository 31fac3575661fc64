"""The child process of tests/test_gpu_ntt_planted.py: BFS_NTT_STREAMING and BFS_NTT_PIPELINE are read once per process, so each of
the two routes gets a process of its own, run once by the parent, which sets the switch.

  python ntt_planted_child.py streaming INPUTS_DIR   every multi-pass planted case, one call each (BFS_NTT_STREAMING=1: the non-temporal
                                                     instantiations of every tile kernel, otherwise reached only above 128 MiB per call)
  python ntt_planted_child.py pipeline INPUTS_DIR    the planted columns of one size, root and direction as ONE batch (BFS_NTT_PIPELINE=
                                                     force: the column pipeline, and pass 0's loads-only non-temporal instantiation)

One JSON line per call: which columns equal the oracle's output bit for bit.  Before each call the child writes "case NAME" to stderr,
where the library's BFS_NTT_PLAN_LOG lines go, so that the parent can tell which route the call took.  INPUTS_DIR: where the parent's
tests left the inputs they built (tests/ntt_planted.py: build_case); what is not there is built here."""
import json
import sys

import numpy as np

from ntt_pipeline_child import FILL, Buf, lib, mark, ntt, o          # (also puts the repository root on sys.path)
from stark_brainfuck_amd import _lib

import ntt_planted as planted


def run(name, cases, inputs_dir):
    """the columns of `cases` (same size and call) as one out-of-place batch"""
    built = [planted.build_case(o, c, inputs_dir=inputs_dir) for c in cases]
    logn, call = cases[0].logn, built[0].call
    assert all(c.logn == logn and c.batch == 1 for c in cases) and all(b.call == call for b in built)
    n, batch = 1 << logn, len(cases)
    din, dout = Buf(batch * n, 0), Buf(batch * n, FILL)
    din.put(np.concatenate([b.x for b in built]))
    mark(name)
    ntt(din.ptr, n, n, dout.ptr, n, logn, batch, call[0], call[1], call[2])
    _lib.check(lib.bfs_stream_synchronize(None))
    got = dout.get()
    print(json.dumps({"case": name, "columns": [planted.case_id(c) for c in cases],
                      "oracle": [bool((got[k * n:(k + 1) * n] == b.want).all()) for k, b in enumerate(built)]}), flush=True)
    dout.free()
    din.free()


if __name__ == "__main__":
    try:
        what, inputs_dir = sys.argv[1], sys.argv[2]
        if what == "streaming":
            for c in planted.MULTI_PASS_CASES:
                run(planted.case_id(c), [c], inputs_dir)
        else:
            for name, cases in planted.column_groups():
                run(name, cases, inputs_dir)
        print(json.dumps({"done": True}), flush=True)
    except Exception as e:                                               # noqa: BLE001
        print(json.dumps({"error": repr(e)}), flush=True)
        raise
