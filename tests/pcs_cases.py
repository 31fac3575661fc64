"""Operands and protocol cases that tests/test_pcs_host.py (emulated kernels, host verifier) and tests/test_gpu_pcs.py (the kernels, the
prover) share.  No test lives here."""
import functools

import numpy as np

import field_states
import pcs_model as model

P = model.P
OFFSET = 7
SEED = 0x0DEE9
OUTSIDE = 0x1234567890ABCDEF % P                     # a lifted base value that is not offset * omega^i for any domain used here
# 0, 1, a lifted base value outside the domain, a genuine extension element with limbs p - 1
POINTS = ((0, 0, 0), (1, 0, 0), (OUTSIDE, 0, 0), (P - 1, P - 1, P - 1))
# every length at which the evaluation kernel takes another path: one thread, a thread stripe (256) +- 1, a workgroup (16384) +- 1
EVAL_LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 16383, 16384, 16385)
EVAL_BATCHES = (1, 3, 7)
POINT_COUNTS = (1, 2, 4)
QUOTIENT_SIZES = (8, 64, 256)
LAYOUTS = {"base": (0, 1), "ext": (1, 0), "mixed": (2, 3)}          # name -> (extension columns, base columns)


def carry_values():
    """tests/field_states.py's carry-reaching residues: the palette and the operands of the fused-product witnesses"""
    values = list(field_states.PALETTE) + [v for pair in field_states.FUSED_WITNESSES for v in pair]
    return [v for v in values if v < P]


def plant(words, step=1):
    """carry-reaching values at the front of a 1-D array (every `step`-th word) and at its end"""
    values = carry_values()
    for k, v in enumerate(values):
        if k * step < words.size:
            words[k * step] = v
    words[-1] = P - 1
    return words


@functools.lru_cache(maxsize=None)
def eval_case(n, stride=None):
    """-> (coefficients (7, stride) with junk behind n, points, reference[b][j] = column b at points[j]); computed once, shared, never
    changed.  points: the genuine extension element first, so that it is the point of k = 1"""
    from oracle import ref_oracle as o
    stride = n if stride is None else stride
    coeffs = o.felt_array(SEED + n, 0, 7 * stride).reshape(7, stride).copy()
    for b in range(7):
        plant(coeffs[b, :n], step=1 + b)
    batch = 7 if n <= 1000 else 1                    # the long lengths: one column, one point on the CPython side
    points = POINTS[::-1] if n <= 1000 else POINTS[3:]
    reference = [[model.evaluate_base(coeffs[b, :n], z) for z in points] for b in range(batch)]
    coeffs.setflags(write=False)
    return coeffs, points, reference


def eval_shapes(n):
    """(batch, k) combinations compared at length n: the first `batch` columns at the first k points of the case"""
    if n > 1000:
        return [(1, 1)]
    return [(batch, k) for batch in EVAL_BATCHES for k in POINT_COUNTS]


@functools.lru_cache(maxsize=None)
def quotient_case(N, layout, k, stride=None):
    """-> dict(columns: per column a (N,) or (3, stride) array, extension columns first; points, values, lam, omega, g: the model's)"""
    from oracle import ref_oracle as o
    n_ext, n_base = LAYOUTS[layout]
    stride = N if stride is None else stride
    seed = SEED + 31 * N + 7 * k + n_ext
    columns = []
    for c in range(n_ext):
        soa = o.felt_array(seed, 1000 * c, 3 * stride).reshape(3, stride).copy()
        for limb in range(3):
            plant(soa[limb, :N], step=1 + limb)
        columns.append(soa)
    for c in range(n_base):
        columns.append(plant(o.felt_array(seed, 50000 + 1000 * c, N).copy(), step=2))
    carry = carry_values()
    points = list(POINTS[4 - k:])                      # k = 1: the genuine extension element; k = 4: all four
    values = [tuple(carry[(3 * j + l + N) % len(carry)] for l in range(3)) for j in range(k)]
    lam = (carry[-1], int(o.felt(seed, 7)), carry[3])
    omega = o.primitive_nth_root(N)
    g = model.quotient(columns, N, OFFSET, omega, points, values, lam)
    for c in columns:
        c.setflags(write=False)
    g.setflags(write=False)
    return {"columns": columns, "points": points, "values": values, "lam": lam, "omega": omega, "g": g, "n_ext": n_ext, "stride": stride}


# ---- protocol cases: (N, folding factor, coset leaves, grinding bits), expansion 4, t = 2
EXPANSION, T = 4, 2
MODES = {"default": (2, False, 0), "fold4": (4, False, 0), "coset8": (8, True, 4)}


def polynomials(o, N, zero=False):
    """one extension polynomial of d coefficients; three base polynomials: d coefficients, d - 3, a constant (zero: the zero polynomial
    in the constant's place)"""
    d = N // EXPANSION
    ext = o.felt_array(SEED + N, 0, 3 * d).reshape(3, d).copy()
    ext[0, 0], ext[1, d - 1] = 0, P - 1
    base = [o.felt_array(SEED + N, 10000, d).copy(), o.felt_array(SEED + N, 20000, d - 3).copy(), np.array([0 if zero else P - 2], dtype=np.uint64)]
    return [ext], base


def protocol_points(o, N, k, seed=0):
    """z and omega^(N / 64) * z for a genuine extension element z"""
    z = tuple(int(v) for v in o.felt_array(SEED + N + 977 * seed, 30000, 3))
    w = pow(o.primitive_nth_root(N), N // 64, P)
    return [z, tuple(v * w % P for v in z)][:k]


@functools.lru_cache(maxsize=None)
def model_proof(N, mode, k, zero=False, forced=False, seed=0, repeated=False):
    """the model's commitment and opening -- computed once per case, shared, never changed.  repeated: the first point k times (the
    model has no rule against a point that is given twice)"""
    from oracle import ref_oracle as o
    a, coset, bits = MODES[mode]
    omega = o.primitive_nth_root(N)
    ext, base = polynomials(o, N, zero)
    committed = model.commit(o, ext, base, N, OFFSET, omega)
    points = protocol_points(o, N, k, seed)
    if repeated:
        points = points[:1] * k
    forced_values = None
    if forced:
        forced_values = model.true_values(committed, points)
        forced_values[-1][1] = model.xadd(forced_values[-1][1], (1, 0, 0))
    out = model.open(o, committed, points, OFFSET, omega, EXPANSION, T, a, coset, bits, forced_values=forced_values)
    out.update(root=committed["root"], ext=ext, base=base, omega=omega, N=N, mode=mode)
    return out
