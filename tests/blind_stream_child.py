"""Child process of tests/test_gpu_blind_kernels.py: the two entry points of include/bfstark_blind.h through the two legs of
tests/stream_order_child.py (its Runner, with tests/stream_hold.py, both imported as they are) -- on a held stream behind the upload that
replaces decoy operands, and on a free stream while the default stream is held.  A call that ran ahead of its stream would blind the
decoy's words.  bfsz_poly_blind works in place on 27 rows of 64 + 14 coefficients 83 words apart; bfsz_split_blind cuts 512 coefficients
into 11 segments of 47 + 17 words.  The references are the integer models of tests/blind_cases.py.  One JSON line per control and case.

    python tests/blind_stream_child.py [--chain K]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (HERE, os.path.dirname(HERE)):
    if path not in sys.path:
        sys.path.insert(0, path)

import blind_cases as bc                       # noqa: E402
import stream_cases as sc                      # noqa: E402
from stream_hold import CHAIN, HipError        # noqa: E402
from stream_order_child import Runner, emit    # noqa: E402

BATCH, H, K, STRIDE, BLIND_STRIDE = 27, 64, 14, 83, 17
S, L0, M, SEGMENTS, H_STRIDE, B_STRIDE, OUT_STRIDE = 512, 47, 17, 11, 515, 19, 69
assert STRIDE >= H + K and BLIND_STRIDE >= K and SEGMENTS * L0 >= S and OUT_STRIDE >= L0 + M


def blind_cases():
    def poly_call(lib, buf, stream, v):
        sc.ck(lib, lib.bfsz_poly_blind(buf["io"], STRIDE, H, BATCH, buf["blind"], BLIND_STRIDE, K, stream))

    def poly_want(c, inp, v):
        out = inp["io"].copy().reshape(BATCH, STRIDE)          # the gaps keep what the input held there
        blind = inp["blind"].reshape(BATCH, BLIND_STRIDE)
        for b in range(BATCH):
            out[b, :H + K] = np.array(bc.poly_blind_model([int(x) for x in out[b, :H + K]], [int(x) for x in blind[b, :K]], H, K), dtype=np.uint64)
        return {"io": out.reshape(-1)}

    def split_call(lib, buf, stream, v):
        sc.ck(lib, lib.bfsz_split_blind(buf["h"], H_STRIDE, S, L0, SEGMENTS, buf["b"], B_STRIDE, M, buf["out"], OUT_STRIDE, stream))

    def split_want(c, inp, v):
        planes = [[int(x) for x in inp["h"][l * H_STRIDE:l * H_STRIDE + S]] for l in range(3)]
        b = [[[int(x) for x in inp["b"][(3 * j + l) * B_STRIDE:(3 * j + l) * B_STRIDE + M]] for l in range(3)] for j in range(SEGMENTS - 1)]
        out = np.zeros((3 * SEGMENTS, OUT_STRIDE), dtype=np.uint64)
        for j, segment in enumerate(bc.split_blind_model(planes, S, L0, SEGMENTS, b, M)):
            for l, row in enumerate(segment):
                out[3 * j + l, :L0 + M] = np.array(row, dtype=np.uint64)
        return {"out": out.reshape(-1)}
    return [sc.Case("poly_blind, 27 rows in place, k = 14", "enqueues", ["bfsz_poly_blind"],
                    lambda c, v: {"io": c.felt(v, 0, BATCH * STRIDE), "blind": c.felt(v, 1, BATCH * BLIND_STRIDE)},
                    poly_call, poly_want, outputs={"io": BATCH * STRIDE}, select={"io": sc.rows_index(BATCH, STRIDE, H + K)}),
            sc.Case("split_blind, 11 segments of 47 + 17 words", "enqueues", ["bfsz_split_blind"],
                    lambda c, v: {"h": c.felt(v, 0, 3 * H_STRIDE), "b": c.felt(v, 1, 3 * (SEGMENTS - 1) * B_STRIDE)},
                    split_call, split_want, outputs={"out": 3 * SEGMENTS * OUT_STRIDE},
                    select={"out": sc.rows_index(3 * SEGMENTS, OUT_STRIDE, L0 + M)})]


def main(argv):
    chain = int(argv[argv.index("--chain") + 1]) if "--chain" in argv else CHAIN
    from stark_brainfuck_amd import _lib
    lib = _lib.load()
    try:
        run = Runner(lib, chain)
        if not run.control_streams_are_independent():
            emit(error="the streams of this process are not independent: leg 2 cannot be judged")
            return 1
        for case in blind_cases():
            run.run_case(case)
        emit(done=True)
        return 0
    except (HipError, RuntimeError) as e:
        emit(error=str(e))
        return 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
