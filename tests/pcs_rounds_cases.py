"""Operands, plans and protocol cases that tests/test_pcs_rounds_host.py (emulated launches, host verifier) and
tests/test_gpu_pcs_rounds.py (the library, the prover) share: openings across commitments over tests/pcs_cases.py's planted operands.
Every plan is chosen so that one clause of the split rule (csrc/deep_core.hpp: deep_rounds_split) closes a launch; the expected launches
are stated by tests/pcs_rounds_model.py's restatement of the rule.  No test lives here."""
import functools

import numpy as np

import pcs_cases
import pcs_groups_cases as gcases
import pcs_groups_model as gmodel
import pcs_model as model
import pcs_rounds_model as rmodel

P = model.P
OFFSET, SEED = pcs_cases.OFFSET, 0x120D5
# 2: fewer points than a thread's share; 512 and 1024: one and two points of the domain per thread where a thread takes two (up to four
# distinct points in the launch), two and four workgroups where it takes one
SIZES = (2, 64, 512, 1024)
CASE_SIZES = {"fits": SIZES + (1 << 12,), "by_columns": SIZES, "by_groups": SIZES, "by_points": SIZES, "by_pairs": SIZES, "rounds3": SIZES,
              "max": (64, 512)}                       # (the Python-int model of 96 columns bounds the sizes of `max`)
ALL = [(name, N) for name in sorted(CASE_SIZES) for N in CASE_SIZES[name]]
IDS = ["%s-%d" % c for c in ALL]
ROUNDS3 = ((5, 11), (9, 0), (0, 7))                   # (extension, base) columns of three commitments: the shape a STARK makes


def _round_columns(o, seed, rounds, N, stride):
    """the columns of commitments of (extension, base) widths `rounds`, in global order: every commitment its extension columns first"""
    columns = []
    for r, (n_ext, n_base) in enumerate(rounds):
        columns += gcases._columns(o, seed + 7919 * r, n_ext, n_base, N, stride)
    return columns


def _points(o, seed, count):
    return gcases.random_points(o, seed, count)


def _case(o, name, N, rounds, stride, raw_plan, want_launches):
    seed = SEED + 31 * N + sum(ord(ch) for ch in name)
    columns = _round_columns(o, seed, rounds, N, stride)
    plan = gmodel.Plan(raw_plan)
    assert plan.m == len(columns)
    launches = rmodel.launches(plan)
    assert launches == want_launches, (name, launches)
    carry = pcs_cases.carry_values()
    lam = (carry[2], int(o.felt(seed, 7)), carry[-1])
    case = gcases._finish(o, N, columns, None, stride, plan, gcases._pair_values(plan, N), lam)
    case.update(launches=launches, rounds=rounds, name=name)
    return case


@functools.lru_cache(maxsize=None)
def case(name, N, stride=None):
    """-> dict(columns in global order, stride, plan, Y, lam, omega, g: the model's, N, launches: the rule's, per launch its groups)"""
    from oracle import ref_oracle as o
    stride = N if stride is None else stride
    if name == "fits":              # tests/pcs_groups_cases.py's tables plan as one round of 3 + 4 columns: one launch
        out = dict(gcases.plan_tables(N) if stride == N else gcases.plan_tables(N, stride=stride))
        out.update(launches=rmodel.launches(out["plan"]), rounds=((3, 4),), name=name)
        assert out["launches"] == [[0, 1, 2]]
        return out
    z = _points(o, 11 * N + len(name), 9)
    if name == "by_columns":        # a one-column group, then a 32-column group: the column limit closes the first launch
        return _case(o, name, N, ((2, 15), (3, 13)), stride, [([0], [z[0]]), (list(range(1, 33)), [z[0], z[1]])], [[0], [1]])
    if name == "by_groups":         # 9 single-column groups at one point
        return _case(o, name, N, ((2, 3), (1, 3)), stride, [([c], [z[0]]) for c in range(9)], [list(range(8)), [8]])
    if name == "by_points":         # 9 groups at 9 different points: 8 distinct points (one point per thread), then 1 (two per thread)
        return _case(o, name, N, ((1, 3), (2, 3)), stride, [([c], [z[c]]) for c in range(9)], [list(range(8)), [8]])
    if name == "by_pairs":          # 5 groups of four points each: 20 pairs
        return _case(o, name, N, ((2, 4), (1, 3)), stride, [([2 * g, 2 * g + 1], z[:4]) for g in range(5)], [[0, 1, 2, 3], [4]])
    if name == "rounds3":
        return _case(o, name, N, ROUNDS3, stride, rounds3_plan(z[0], z[1], z[2], z[3]), [[0, 1, 2, 3]])
    assert name == "max"            # 96 columns (16 + 16 extension), 24 groups, 24 distinct points, 48 pairs; a one-column group
    pts = _points(o, 13 * N, 24)
    sizes = [1, 7] + [4] * 22
    order = [37 * c % 96 for c in range(96)]
    groups, at = [], 0
    for g, size in enumerate(sizes):
        groups.append((sorted(order[at:at + size]), [pts[g], pts[(g + 1) % 24]]))
        at += size
    plan = gmodel.Plan(groups)
    assert (plan.m, len(plan.groups), len(plan.points), sum(len(i) for _, i in plan.groups)) == (96, 24, 24, 48)
    # eight distinct points close the first three launches after seven groups each; the last has four: two points per thread again
    return _case(o, name, N, ((16, 16), (16, 16), (0, 32)), stride, groups, [list(range(0, 7)), list(range(7, 14)), list(range(14, 21)), [21, 22, 23]])


def rounds3_plan(z, wz, w2z, w3z):
    """three commitments of 5 + 11, 9 + 0 and 0 + 7 columns (global columns 0..15, 16..24, 25..31): three tables whose base columns (first
    commitment, columns 5..15) and extension columns (its columns 0..4 and the second commitment) are wanted at z and at the table's own
    next row, and the third commitment's quotient columns at z only"""
    return [([0, 1, 2, 5, 6, 7, 16, 17, 18], [z, wz]), ([3, 4, 8, 9, 10, 19, 20, 21, 22], [z, w2z]), ([11, 12, 13, 14, 15, 23, 24], [z, w3z]),
            (list(range(25, 32)), [z])]


def kernel_arguments(case):
    """what bfsr_deep_quotient_rounds takes (tests/pcs_groups_cases.py: kernel_arguments, the same layout)"""
    return gcases.kernel_arguments(case)


# ---- protocol cases: expansion 4, t = 2; the default mode at N = 64, folding_factor = 8 with coset leaves (and 4 grinding bits) at 256
EXPANSION, T, MODES = pcs_cases.EXPANSION, pcs_cases.T, pcs_cases.MODES
PROTOCOL = [(64, "default"), (256, "coset8")]
PROTOCOL_IDS = ["%d-%s" % c for c in PROTOCOL]
INTERLUDES = ([7, 8], (9,))                           # what the caller pushes between the rounds' commitments
ROOT_AT, START = (0, 2, 4), 5                         # where the three roots lie in the stream; where the opening begins
# A forced proof is honest except for ONE false value (group 1, its second point, its first column -- a column of the FIRST commitment).
# With t = 2 the low-degree test catches a false claim only with some probability, so the seed of the points is fixed per case such
# that the MODEL's verifier refuses (searched on the CPU from 0 upwards; tests/test_pcs_rounds_host.py checks it).
FORCED_SEEDS = {(64, "default"): 0, (256, "coset8"): 0}


def polynomials(o, N):
    """per commitment of ROUNDS3 (extension polynomials, base polynomials): d coefficients, some d - 3, one constant"""
    d = N // EXPANSION
    out = []
    for r, (n_ext, n_base) in enumerate(ROUNDS3):
        ext = [o.felt_array(SEED + N + r, 3000 * c, 3 * (d - 3 * (c % 2))).reshape(3, d - 3 * (c % 2)).copy() for c in range(n_ext)]
        base = [o.felt_array(SEED + N + r, 100000 + 3000 * c, d - 3 * (c % 2)).copy() for c in range(n_base)]
        if base:
            base[-1] = np.array([P - 2 - r], dtype=np.uint64)
        if ext:
            ext[0][0, 0], ext[0][1, d - 1] = 0, P - 1
        out.append((ext, base))
    return out


def protocol_plan(o, N, seed=0):
    z = gcases.random_points(o, N + 977 * seed + 5, 1)[0]
    omega = o.primitive_nth_root(N)
    nexts = [tuple(v * pow(omega, N // 64 << i, P) % P for v in z) for i in range(3)]
    return rounds3_plan(z, *nexts)


def single_plan(o, N):
    """the first commitment of ROUNDS3 alone (16 columns): what open_at takes too"""
    z = gcases.random_points(o, N + 3, 2)
    return [([0, 1, 5, 6, 7], [z[0], z[1]]), ([2, 3, 4] + list(range(8, 16)), [z[0]])]


@functools.lru_cache(maxsize=None)
def model_proof(N, mode, forced=False, seed=0, single=False):
    """the model's commitments in rounds (the interludes pushed between them) and its one opening -- computed once per case, shared,
    never changed"""
    from oracle import ref_oracle as o
    a, coset, bits = MODES[mode]
    omega = o.primitive_nth_root(N)
    polys = polynomials(o, N)[:1 if single else None]
    ps = o.ProofStreamOracle()
    commitments = []
    for r, (ext, base) in enumerate(polys):
        commitments.append(rmodel.commit(o, ext, base, N, OFFSET, omega, ps))
        if r < len(polys) - 1:
            ps.push(INTERLUDES[r])
    raw_plan = single_plan(o, N) if single else protocol_plan(o, N, seed)
    plan = gmodel.Plan(raw_plan)
    forced_values = None
    if forced:
        forced_values = rmodel.true_values(commitments, plan)
        forced_values[1][1][0] = model.xadd(forced_values[1][1][0], (1, 0, 0))
    out = rmodel.open(o, commitments, plan, OFFSET, omega, EXPANSION, T, a, coset, bits, forced_values=forced_values)
    assert single or (out["start"] == START and [ps.objects[at] for at in ROOT_AT] == [c["root"] for c in commitments])
    out.update(roots=[c["root"] for c in commitments], polys=polys, omega=omega, N=N, mode=mode, raw_plan=raw_plan)
    return out
