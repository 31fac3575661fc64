"""Child process of tests/test_gpu_deep_segmented.py: the entry point of include/bfstark_segments.h through the two legs of
tests/stream_order_child.py (its Runner, with tests/stream_hold.py, both imported as they are) -- on a held stream behind the upload that
replaces decoy codewords, and on a free stream while the default stream is held.  A call that ran ahead of its stream would gather the
decoy's words.  27 rows of 257 words from rows 1031 words apart, every fourth word, into rows 263 words apart; the reference is numpy
slicing.  One JSON line per control and case.

    python tests/deep_segments_stream_child.py [--chain K]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (HERE, os.path.dirname(HERE)):
    if path not in sys.path:
        sys.path.insert(0, path)

import stream_cases as sc                      # noqa: E402
from stream_hold import CHAIN, HipError        # noqa: E402
from stream_order_child import Runner, emit    # noqa: E402

BATCH, N_OUT, LOG_STEP, STRIDE_IN, STRIDE_OUT = 27, 257, 2, 1031, 263
assert STRIDE_IN >= ((N_OUT - 1) << LOG_STEP) + 1 and STRIDE_OUT > N_OUT


def segments_cases():
    def call(lib, buf, stream, v):
        sc.ck(lib, lib.bfsg_decimate_rows(buf["in"], STRIDE_IN, LOG_STEP, buf["out"], STRIDE_OUT, N_OUT, BATCH, stream))

    def want(c, inp, v):
        out = np.zeros((BATCH, STRIDE_OUT), dtype=np.uint64)
        out[:, :N_OUT] = inp["in"].reshape(BATCH, STRIDE_IN)[:, ::1 << LOG_STEP][:, :N_OUT]
        return {"out": out.reshape(-1)}
    return [sc.Case("decimate_rows, 27 rows, every fourth word", "enqueues", ["bfsg_decimate_rows"], lambda c, v: {"in": c.felt(v, 0, BATCH * STRIDE_IN)},
                    call, want, outputs={"out": BATCH * STRIDE_OUT})]


def main(argv):
    chain = int(argv[argv.index("--chain") + 1]) if "--chain" in argv else CHAIN
    from stark_brainfuck_amd import _lib
    lib = _lib.load()
    try:
        run = Runner(lib, chain)
        if not run.control_streams_are_independent():
            emit(error="the streams of this process are not independent: leg 2 cannot be judged")
            return 1
        for case in segments_cases():
            run.run_case(case)
        emit(done=True)
        return 0
    except (HipError, RuntimeError) as e:
        emit(error=str(e))
        return 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
