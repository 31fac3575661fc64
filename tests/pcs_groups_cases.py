"""Operands and protocol cases that tests/test_pcs_groups_host.py (emulated kernels, host verifier) and tests/test_gpu_pcs_groups.py (the
kernels, the prover) share: opening plans over tests/pcs_cases.py's operands.  No test lives here."""
import functools

import numpy as np

import pcs_cases
import pcs_groups_model as gmodel
import pcs_model as model

P = model.P
OFFSET, SEED = pcs_cases.OFFSET, 0x6C0DE
# points of the domain one workgroup of the quotient kernel owns, by distinct points of the plan (256 threads, two points each up to
# four distinct points, one above); tests/test_pcs_groups_host.py holds this against the kernel's own constant
SHARE = {n_points: 512 if n_points <= 4 else 256 for n_points in range(1, 9)}
# fewer points than a thread's share; 8; 256; the first N above a workgroup's share (512: one point per thread, 1024: two); several workgroups
QUOTIENT_SIZES = (2, 8, 256, 512, 1024, 1 << 12)
MAX_SIZES = (64, 512)                                # the plan `max`: 8 distinct points, so 512 is two workgroups
POINT_COUNTS = pcs_cases.POINT_COUNTS
LAYOUTS = pcs_cases.LAYOUTS


def random_points(o, seed, count):
    """genuine extension elements (a non-zero third limb): never a point of a domain"""
    words = [int(v) for v in o.felt_array(SEED + seed, 77000, 3 * count)]
    return [(words[3 * j], words[3 * j + 1], words[3 * j + 2] or 1) for j in range(count)]


def _columns(o, seed, n_ext, n_base, N, stride):
    columns = []
    for c in range(n_ext):
        soa = o.felt_array(seed, 1000 * c, 3 * stride).reshape(3, stride).copy()
        for limb in range(3):
            pcs_cases.plant(soa[limb, :N], step=1 + limb)
        columns.append(soa)
    for c in range(n_base):
        columns.append(pcs_cases.plant(o.felt_array(seed, 50000 + 1000 * c, N).copy(), step=2))
    return columns


def _pair_values(plan, N):
    carry = pcs_cases.carry_values()
    at = iter(range(10 ** 6))
    return [[tuple(carry[(3 * next(at) + l + N) % len(carry)] for l in range(3)) for _ in indices] for _, indices in plan.groups]


def _finish(o, N, columns, n_ext, stride, plan, Y, lam, g=None):
    omega = o.primitive_nth_root(N)
    plan = plan if isinstance(plan, gmodel.Plan) else gmodel.Plan(plan)
    if g is None:
        g = gmodel.quotient(columns, N, OFFSET, omega, plan, Y, lam)
    for c in columns:
        c.setflags(write=False)
    g.setflags(write=False)
    return {"columns": columns, "n_ext": n_ext, "stride": stride, "plan": plan, "Y": Y, "lam": lam, "omega": omega, "g": g, "N": N}


@functools.lru_cache(maxsize=None)
def plan_one(N, layout, k, stride=None):
    """a single group of all columns over tests/pcs_cases.py's quotient case: g is pcs_model.quotient's"""
    from oracle import ref_oracle as o
    case = pcs_cases.quotient_case(N, layout, k, stride)
    m = len(case["columns"])
    return _finish(o, N, case["columns"], case["n_ext"], case["stride"], [(list(range(m)), case["points"])], [list(case["values"])], case["lam"], case["g"])


@functools.lru_cache(maxsize=None)
def plan_singletons(N, stride=None):
    """the five columns of the mixed layout, each its own group, all at the one point of k = 1: base[g][0] = g, so g is plan_one's when
    the five Y_g add up to its Y"""
    from oracle import ref_oracle as o
    case = pcs_cases.quotient_case(N, "mixed", 1, stride)
    carry = pcs_cases.carry_values()
    Y = [(carry[(5 * g + 1) % len(carry)], carry[(7 * g + 2) % len(carry)], carry[(11 * g + 3) % len(carry)]) for g in range(4)]
    rest = case["values"][0]
    for y in Y:
        rest = model.xsub(rest, y)
    return _finish(o, N, case["columns"], case["n_ext"], case["stride"], [([c], case["points"]) for c in range(5)], [[y] for y in Y + [rest]], case["lam"],
                   case["g"])


@functools.lru_cache(maxsize=None)
def plan_tables(N, stride=None):
    """3 extension + 4 base columns; z is shared by three groups: 3 distinct points, 5 pairs"""
    from oracle import ref_oracle as o
    stride = N if stride is None else stride
    seed = SEED + 31 * N
    columns = _columns(o, seed, 3, 4, N, stride)
    z = random_points(o, N, 1)[0]
    wz, w2z = tuple(v * OFFSET % P for v in z), tuple(v * pcs_cases.OUTSIDE % P for v in z)
    plan = gmodel.Plan([([0, 3, 4], [z, wz]), ([1, 5], [z, w2z]), ([2, 6], [z])])
    assert len(plan.points) == 3 and plan.base == [[0, 3], [6, 8], [10]]
    carry = pcs_cases.carry_values()
    return _finish(o, N, columns, 3, stride, plan, _pair_values(plan, N), (carry[-1], int(o.felt(seed, 7)), carry[3]))


@functools.lru_cache(maxsize=None)
def plan_max(N, stride=None):
    """every limit at once: 32 columns (8 extension), 8 groups, 8 distinct points, 16 pairs; a four-point group, a one-column group"""
    from oracle import ref_oracle as o
    stride = N if stride is None else stride
    seed = SEED + 37 * N
    columns = _columns(o, seed, 8, 24, N, stride)
    pts = list(pcs_cases.POINTS) + random_points(o, 5 * N, 4)
    groups = [[0, 9, 17], [5]] + [[] for _ in range(6)]
    for at, c in enumerate(c for c in range(32) if c not in (0, 9, 17, 5)):
        groups[2 + at % 6].append(c)
    opened = [[0, 1, 2, 3], [4, 5], [6, 7], [0, 4], [7, 1], [5, 2], [6], [3]]
    plan = gmodel.Plan([(cols, [pts[p] for p in where]) for cols, where in zip(groups, opened)])
    assert len(plan.groups) == 8 and len(plan.points) == 8 and sum(len(i) for _, i in plan.groups) == 16 and plan.m == 32
    carry = pcs_cases.carry_values()
    return _finish(o, N, columns, 8, stride, plan, _pair_values(plan, N), (carry[2], carry[-1], int(o.felt(seed, 9))))


def kernel_arguments(case):
    """what bfsx_deep_quotient_groups takes: the columns in group order, group sizes, the pairs' point indices, the pairs' Y"""
    plan = case["plan"]
    order = [c for columns, _ in plan.groups for c in columns]
    return {"order": order, "columns": [case["columns"][c] for c in order], "group_columns": [len(columns) for columns, _ in plan.groups],
            "group_pairs": [len(indices) for _, indices in plan.groups], "points": plan.points,
            "pair_point": [p for _, indices in plan.groups for p in indices], "pair_values": [y for per_group in case["Y"] for y in per_group]}


# ---- evaluation of separate columns: a column shorter than one workgroup beside one that needs three, every edge of a stripe and of a
# workgroup between them -- all in ONE call; and the two ends of the column count
EVAL_LENGTHS = (1, 255, 256, 257, 16383, 16384, 16385, 2 * 16384 + 1)
EVAL_MANY = tuple(1 + 13 * b % 300 for b in range(96))          # 96 short columns
EVAL_CASES = {"ragged": EVAL_LENGTHS, "one": (257,), "many": EVAL_MANY}
EVAL_POINT_COUNTS = (1, 4)


@functools.lru_cache(maxsize=None)
def eval_case(name):
    """-> (columns: separate 1-D arrays, points (4), reference[b][j]); computed once, shared, never changed"""
    from oracle import ref_oracle as o
    lengths = EVAL_CASES[name]
    columns = [pcs_cases.plant(o.felt_array(SEED + len(lengths), 100000 * b, n).copy(), step=1 + b % 5) for b, n in enumerate(lengths)]
    points = [pcs_cases.POINTS[3], random_points(o, 9, 1)[0], pcs_cases.POINTS[2], pcs_cases.POINTS[0]]
    reference = [[model.evaluate_base(c, z) for z in points] for c in columns]
    for c in columns:
        c.setflags(write=False)
    return columns, points, reference


# ---- protocol cases: expansion 4, t = 2, modes of tests/pcs_cases.py
EXPANSION, T, MODES = pcs_cases.EXPANSION, pcs_cases.T, pcs_cases.MODES
# A forced proof is honest except for ONE false value (group 1, its second point, its first column).  With t = 2 the low-degree test
# catches a false claim only with some probability, so the seed of the points is fixed per case such that the MODEL's verifier refuses
# (searched on the CPU from 0 upwards; tests/test_pcs_groups_host.py checks it).
FORCED_SEEDS = {(64, "default"): 0, (256, "coset8"): 0}


def polynomials(o, N):
    """two extension polynomials (d and d - 3 coefficients), three base polynomials: d coefficients, d - 3, a constant"""
    d = N // EXPANSION
    ext = [o.felt_array(SEED + N, 0, 3 * d).reshape(3, d).copy(), o.felt_array(SEED + N, 5000, 3 * (d - 3)).reshape(3, d - 3).copy()]
    ext[0][0, 0], ext[0][1, d - 1] = 0, P - 1
    base = [o.felt_array(SEED + N, 10000, d).copy(), o.felt_array(SEED + N, 20000, d - 3).copy(), np.array([P - 2], dtype=np.uint64)]
    return ext, base


def protocol_plan(o, N, seed=0):
    """tables-like: row columns 0, 1 extension, 2..4 base; z and omega^(N / 64) z; the second group opens them the other way round"""
    z = random_points(o, N + 977 * seed, 1)[0]
    w = pow(o.primitive_nth_root(N), N // 64, P)
    wz = tuple(v * w % P for v in z)
    return [([0, 2, 4], [z, wz]), ([1], [wz, z]), ([3], [z])]


@functools.lru_cache(maxsize=None)
def model_proof(N, mode, forced=False, seed=0):
    """the model's commitment and opening -- computed once per case, shared, never changed"""
    from oracle import ref_oracle as o
    a, coset, bits = MODES[mode]
    omega = o.primitive_nth_root(N)
    ext, base = polynomials(o, N)
    committed = model.commit(o, ext, base, N, OFFSET, omega)
    plan = gmodel.Plan(protocol_plan(o, N, seed))
    forced_values = None
    if forced:
        forced_values = gmodel.true_values(committed, plan)
        forced_values[1][1][0] = model.xadd(forced_values[1][1][0], (1, 0, 0))
    out = gmodel.open(o, committed, plan, OFFSET, omega, EXPANSION, T, a, coset, bits, forced_values=forced_values)
    out.update(root=committed["root"], ext=ext, base=base, omega=omega, N=N, mode=mode, raw_plan=protocol_plan(o, N, seed))
    return out
