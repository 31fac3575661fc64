"""Child process of tests/test_gpu_pcs_rounds.py: the entry point of include/bfstark_rounds.h, with a plan that needs TWO launches,
through the two legs of tests/stream_order_child.py (its Runner, with tests/stream_hold.py, both imported as they are) -- on a held
stream behind the upload that replaces a decoy input, and on a free stream while the default stream is held.  An accumulating launch
that ran ahead of its stream would add to a quotient that is not there yet.  One JSON line per control and case.

    python tests/pcs_rounds_stream_child.py [--chain K]
"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (HERE, os.path.dirname(HERE)):
    if path not in sys.path:
        sys.path.insert(0, path)

import pcs_groups_model as gmodel              # noqa: E402
import pcs_rounds_model as rmodel              # noqa: E402
import stream_cases as sc                      # noqa: E402
from stream_hold import CHAIN, HipError        # noqa: E402
from stream_order_child import Runner, emit    # noqa: E402

u64, u32 = ctypes.c_uint64, ctypes.c_uint32
K = 2
LOG_N, M_EXT, M_BASE = 10, 1, 8
# nine groups: the ninth starts a second launch (one distinct point there, two in the first: both take two points of the domain per thread)
GROUPS = tuple(([c], [c % 2] if c < 8 else [1]) for c in range(9))


def _triples(c, v, k, count):
    return [tuple(int(x) for x in c.felt(v, 40 + k, 3 * count)[3 * j:3 * j + 3]) for j in range(count)]


def rounds_case():
    from stark_brainfuck_amd import _lib
    n = 1 << LOG_N
    m = M_EXT + M_BASE
    words = (3 * M_EXT + M_BASE) * n
    pairs = sum(len(indices) for _, indices in GROUPS)

    def host_args(c, v):
        pts = [(z[0], z[1], z[2] or 1) for z in _triples(c, v, 0, K)]          # genuine extension elements: never a point of the domain
        return pts, _triples(c, v, 1, pairs), _triples(c, v, 2, 1)[0]

    def columns(flat):
        return [flat[:3 * n].reshape(3, n)] + [flat[(3 + b) * n:(4 + b) * n] for b in range(M_BASE)]

    def plan_of(pts):
        return gmodel.Plan([(group, [pts[p] for p in indices]) for group, indices in GROUPS])

    def call(lib, buf, stream, v):
        pts, values, lam = host_args(CASE, v)
        cols = (_lib.RowColumn * m)()
        for at, p in enumerate(p for group, _ in GROUPS for p in group):
            cols[at].d_values, cols[at].is_ext, cols[at].field_id = buf["codewords"] + 8 * n * (3 * p if p < M_EXT else 3 * M_EXT + p - M_EXT), int(p < M_EXT), 1
        launches = u32(0)
        sc.ck(lib, lib.bfsr_deep_quotient_rounds(cols, m, n, LOG_N, sc.OFFSET, sc.oracle().primitive_nth_root(n), (u32 * len(GROUPS))(*[len(g) for g, _ in GROUPS]),
                                                 (u32 * len(GROUPS))(*[len(i) for _, i in GROUPS]), len(GROUPS), (u64 * (3 * K))(*[x for z in pts for x in z]), K,
                                                 (u32 * pairs)(*[p for _, i in GROUPS for p in i]), (u64 * (3 * pairs))(*[x for y in values for x in y]),
                                                 (u64 * 3)(*lam), buf["g"], n, ctypes.byref(launches), stream))
        if launches.value != 2:
            raise RuntimeError("the plan of the stream case took %d launches, not 2" % launches.value)

    def want(c, inp, v):
        pts, values, lam = host_args(c, v)
        plan = plan_of(pts)
        assert len(rmodel.launches(plan)) == 2
        Y, at = [], 0
        for _, indices in GROUPS:
            Y.append(values[at:at + len(indices)])
            at += len(indices)
        return {"g": gmodel.quotient(columns(inp["codewords"]), n, sc.OFFSET, sc.oracle().primitive_nth_root(n), plan, Y, lam)}
    CASE = sc.Case("deep_quotient_rounds", "enqueues", ["bfsr_deep_quotient_rounds"], lambda c, v: {"codewords": c.felt(v, 0, words)}, call, want,
                   outputs={"g": 3 * n})
    return CASE


def main(argv):
    chain = int(argv[argv.index("--chain") + 1]) if "--chain" in argv else CHAIN
    from stark_brainfuck_amd import _lib
    lib = _lib.load()
    try:
        run = Runner(lib, chain)
        if not run.control_streams_are_independent():
            emit(error="the streams of this process are not independent: leg 2 cannot be judged")
            return 1
        run.run_case(rounds_case())
        emit(done=True)
        return 0
    except (HipError, RuntimeError) as e:
        emit(error=str(e))
        return 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
