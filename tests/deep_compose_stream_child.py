"""Child process of tests/test_gpu_deep_stark.py: the two entry points of include/bfstark_compose.h through the two legs of
tests/stream_order_child.py (its Runner, with tests/stream_hold.py, both imported as they are) -- on a held stream behind the upload that
replaces decoy codewords and a decoy accumulator, and on a free stream while the default stream is held.  Both calls ADD to an
accumulator: one that ran ahead of its stream would add to values that are not there yet.  The operands are those of the air_combine
cases of tests/stream_cases.py (the memory table at 2^9 points), the reference is tests/test_gpu_pointwise_edges.py's quotients on
Python integers.  One JSON line per control and case.

    python tests/deep_compose_stream_child.py [--chain K]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (HERE, os.path.dirname(HERE)):
    if path not in sys.path:
        sys.path.insert(0, path)

import stream_cases as sc                      # noqa: E402
from stream_hold import CHAIN, HipError        # noqa: E402
from stream_order_child import Runner, emit    # noqa: E402

N, LOG_N = sc.N, sc.LOG_N


def _betas(c, v, count):
    s = sc.scalars(c, v, 2, 3 * count)
    return [tuple(s[3 * k:3 * k + 3]) for k in range(count)]


def compose_cases():
    pe, shape = sc.pointwise, sc.air_shape()

    def air_call(lib, buf, stream, v):
        sh, ops = sc.air_ops(AIR, None, v)
        sc.ck(lib, lib.bfsc_air_compose(sc.AIR_TABLE, buf["base"], buf["ext"], *sc.air_args(sh, ops), sc.flat3(_betas(AIR, v, sh.nq)), 0, 1, buf["acc"], stream))

    def air_want(c, inp, v):
        sh, ops = sc.air_ops(c, inp, v)
        acc = sc.triple_planes(inp["acc"])
        for beta, q in zip(_betas(c, v, sh.nq), pe().quotients(sh, ops, ops.params)):
            acc = pe().xadd(acc, pe().xmul(beta, q))
        return {"acc": sc.words_of(acc)}
    AIR = sc.Case("air_compose onto an accumulator, memory table", "enqueues", ["bfsc_air_compose"],
                  lambda c, v: {"base": c.felt(v, 0, shape.bw * N), "ext": c.felt(v, 1, 3 * shape.xw * N), "acc": c.felt(v, 3, 3 * N)}, air_call, air_want,
                  outputs={"acc": 3 * N})

    def difference_call(lib, buf, stream, v):
        sc.ck(lib, lib.bfsc_difference_compose(buf["lhs"], buf["rhs"], LOG_N, sc.OFFSET, pe().OMEGA, sc.flat3(_betas(DIFFERENCE, v, 1)), 0, 1, buf["acc"], stream))

    def difference_want(c, inp, v):
        lhs, rhs = sc.triple_planes(inp["lhs"]), sc.triple_planes(inp["rhs"])
        q = pe().xscale(tuple((a - b) % sc.P for a, b in zip(lhs, rhs)), pe().inverses(sc.points() - 1))
        return {"acc": sc.words_of(pe().xadd(sc.triple_planes(inp["acc"]), pe().xmul(_betas(c, v, 1)[0], q)))}
    DIFFERENCE = sc.Case("difference_compose onto an accumulator", "enqueues", ["bfsc_difference_compose"],
                         lambda c, v: {"lhs": c.felt(v, 0, 3 * N), "rhs": c.felt(v, 1, 3 * N), "acc": c.felt(v, 2, 3 * N)}, difference_call, difference_want,
                         outputs={"acc": 3 * N})
    return [AIR, DIFFERENCE]


def main(argv):
    chain = int(argv[argv.index("--chain") + 1]) if "--chain" in argv else CHAIN
    from stark_brainfuck_amd import _lib
    lib = _lib.load()
    try:
        run = Runner(lib, chain)
        if not run.control_streams_are_independent():
            emit(error="the streams of this process are not independent: leg 2 cannot be judged")
            return 1
        for case in compose_cases():
            run.run_case(case)
        emit(done=True)
        return 0
    except (HipError, RuntimeError) as e:
        emit(error=str(e))
        return 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
