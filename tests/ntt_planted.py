"""Inputs that put CHOSEN operands in front of the butterflies of any register stage of any pass of the NTT tile kernels.

Values next to 0 and p in a transform's input (edge_values, all p - 1, alternating 1 / p - 1) reach the first butterfly block of the
first pass only: after the first inner twiddle the operands are uniform again and an unreduced sum (gl.hpp: gl_add_lazy) is really
>= p about once in 2^32.  Every stage is linear and invertible, though, so the input that produces a chosen vector at an inner site
can be computed exactly.  A SITE is (pass, stage): the registers of every thread immediately before the butterflies of register stage
`stage` of pass `pass` (csrc/ntt_core.hpp: BFS_NTT_SITE), n words per column in the emulation's call order.  A case is
(log n, root, direction, site, seed):

  1. V: n words per column drawn from a palette of canonical residues next to 0, 2^32, 2^63 and p (tests/field_states.py: PALETTE, its
     negatives, and 2^32 +- 1, p - 2^32, 2^63 +- 1), a sub-palette per group of sixteen words -- one butterfly block of the widest radix;
  2. the host emulation of the kernels (tests/emu/emu_ntt.cpp) transforms a ZERO input with V planted at the site: y, the image of V
     under everything from the site on;
  3. x = the oracle's inverse of the call applied to y  (forward: intt; inverse with n^-1: ntt; full-size coset evaluation with shift 7:
     fast_coset_interpolate);
  4. the expected output is the oracle's transform of x -- computed from x alone.  Nothing of the emulation enters it: the emulation
     only finds x, and tests/test_ntt_planted_host.py checks that x really makes V appear at the site (a recording run), word for word.

Sizes: the smallest that reach every instance of the tile kernels the planner uses for full-size transforms up to 2^20 (PLAN below;
tests/test_ntt_planted_host.py holds the table against the planner).  Below 2^8 one column has too few butterfly blocks to reach every
class of operands, so those cases are batches of columns, each column drawn with a seed of its own.

Left out: PASS_EXPAND and zero-padded inputs -- a zero-padded input is a constraint on x that the inversion cannot keep, so the inner
sites of those plans cannot be reached this way; and the 8-bit digits of balanced three-pass plans, which first occur at 2^22 .. 2^24.

tests/test_gpu_ntt_planted.py gives the same x to bfs_gl_ntt and compares with the oracle, bit for bit."""
import collections
import ctypes
import os
import sys

import numpy as np

from field_states import PALETTE, P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "emu")
u64, u32, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p

COLUMN, SINGLE, FIRST, EXPAND = 0, 1, 2, 3          # csrc/ntt_core.hpp: PASS_*
CHAIN, BALANCED = 0, 1                              # PassArgs::sched
COSET_SHIFT = 7

# ------------------------------------------------------------------------------------------------ the palette
VALUES = tuple(sorted(set(PALETTE) | {(P - v) % P for v in PALETTE} |
                      {(1 << 32) - 1, (1 << 32) + 1, P - (1 << 32), (1 << 63) - 1, (1 << 63) + 1}))
assert all(v < P for v in VALUES)
# one of these per group of sixteen words: everything; next to 0 and p (sums of exactly p, p + 1, 2p - 2, 2p); around 2^32 and
# p - 2^32 (carries between the two 32-bit words); around 2^63 (sums that wrap 2^64 with room to spare)
SUBPALETTES = (
    VALUES,
    (0, 1, 2, P - 2, P - 1),
    (0, 1, P - 1, 0xFFFFFFFF, 0x100000000, 0x100000001, P - 0xFFFFFFFF, P - 0x100000000, P - 0x100000001, 0xFFFFFFFE00000000),
    (0, 1, P - 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, 0x7FFFFFFF00000000, P - (1 << 63), P - (1 << 63) + 1),
)
assert all(v in VALUES for sub in SUBPALETTES for v in sub)
SUBPALETTE_WEIGHTS = (0.25, 0.45, 0.2, 0.1)


def site_vector(n, seed):
    """V for one column: n words (n a multiple of 16), a sub-palette per sixteen; seed: an integer or a list of them"""
    assert n % 16 == 0
    rng = np.random.default_rng(seed)
    groups = n // 16
    kind = rng.choice(len(SUBPALETTES), size=groups, p=SUBPALETTE_WEIGHTS)
    out = np.empty((groups, 16), dtype=np.uint64)
    for k, sub in enumerate(SUBPALETTES):
        rows = np.flatnonzero(kind == k)
        out[rows] = np.array(sub, dtype=np.uint64)[rng.integers(0, len(sub), (len(rows), 16))]
    return out.reshape(n)


# ------------------------------------------------------------------------------------------------ the plans the cases claim to reach
# digits of the plan of a full-size transform, and the twiddle schedule of the three-pass ones (csrc/ntt_plan.hpp: ntt_make_plan)
PLAN = {4: (4,), 5: (5,), 6: (6,), 7: (7,), 8: (8,), 9: (9,), 10: (10,), 11: (11,), 12: (12,),
        13: (7, 6), 14: (7, 7), 15: (8, 7), 16: (8, 8), 17: (6, 6, 5), 18: (6, 6, 6), 19: (7, 6, 6), 20: (7, 7, 6)}
SCHEDULE = {17: CHAIN, 18: BALANCED, 19: BALANCED, 20: BALANCED}
MULTI_PASS = tuple(logn for logn in PLAN if len(PLAN[logn]) > 1)


def stages_of(S):
    """register stages (B1, B2, B3) of a 2^S-row tile (ntt_plan.hpp: ntt_with_tile_shape)"""
    return (4, 0, 0) if S <= 4 else (4, S - 4, 0) if S <= 8 else (4, 4, S - 8)


def claimed_instances(logn):
    """{(mode, S, schedule)} of the steps of a full-size 2^logn transform"""
    digits = PLAN[logn]
    if len(digits) == 1:
        return {(SINGLE, digits[0], CHAIN)}
    return {(FIRST if t == 0 else COLUMN, S, SCHEDULE.get(logn, CHAIN)) for t, S in enumerate(digits)}


Site = collections.namedtuple("Site", "pass_index stage radix_bits lazy canon multiplies")


def sites_of(logn, direction):
    """every (pass, stage) of the plan with what its butterflies are:
    lazy        dif<Q, OUT_LAZY = true>: stage 1 of a tile with more stages, stage 2 of a three-stage tile or of a first pass
    canon       gl_canon runs at the site: the unit-twiddle register of a lazy stage 1, unless n^-1 is folded into that twiddle
    multiplies  the site itself multiplies every output it left unreduced (inner twiddle or store-time row); otherwise the next
                pass' load does"""
    digits = PLAN[logn]
    out = []
    for t, S in enumerate(digits):
        B = stages_of(S)
        U = sum(1 for b in B if b)
        first, last = len(digits) > 1 and t == 0, t + 1 == len(digits)
        for stage in range(1, U + 1):
            lazy = (stage == 1 and U >= 2) or (stage == 2 and (U == 3 or first))
            scaled_unit = direction == "inverse" and last and U == 2          # ntt_pass_args: tw1 = t_in_last, unit0 = 0
            canon = stage == 1 and U >= 2 and not scaled_unit
            multiplies = (stage == 1 and U >= 2) or (stage == 2 and (U == 3 or (first and SCHEDULE.get(logn, CHAIN) == BALANCED)))
            out.append(Site(t, stage, B[stage - 1], lazy, canon, lazy and multiplies))
    return out


# ------------------------------------------------------------------------------------------------ the cases
Case = collections.namedtuple("Case", "logn root_power direction pass_index stage seed batch")
DIRECTIONS = ("forward", "inverse", "coset")
# seeds chosen on the CPU (find_seed below) so that every class of operands tests/test_ntt_planted_host.py asks for occurs at the
# site; cases not named here take seed 1
SEEDS = {"n8-inverse-p0s1": 3, "n8-coset-p0s1": 4}


def batch_of(logn):
    """columns per case: one from 2^8 on, below that as many as make 2^10 words"""
    return 1 if logn >= 8 else 1 << (10 - logn)


def case_id(c):
    return "n%d%s-%s-p%ds%d" % (c.logn, "" if c.root_power == 1 else "-w%d" % c.root_power, c.direction, c.pass_index, c.stage)


def _cases():
    out = []
    for logn in sorted(PLAN):
        for direction in DIRECTIONS:
            for s in sites_of(logn, direction):
                out.append(Case(logn, 1, direction, s.pass_index, s.stage, 0, batch_of(logn)))
    # another primitive root: w^(n/16) = 2^(12 u) with another u, so another u^-1 mod 16 and another register carries the unit twiddle
    for s in sites_of(13, "forward"):
        out.append(Case(13, 3, "forward", s.pass_index, s.stage, 0, 1))
    return [c._replace(seed=SEEDS.get(case_id(c), 1)) for c in out]


CASES = _cases()
CASE_IDS = [case_id(c) for c in CASES]
assert len(set(CASE_IDS)) == len(CASES)


MULTI_PASS_CASES = [c for c in CASES if c.logn in MULTI_PASS]


def column_groups():
    """the multi-pass cases that one call can transform as a batch of columns: same size, root and direction -- one column per site.
    -> [(name, [case, ...])]"""
    groups = collections.OrderedDict()
    for c in MULTI_PASS_CASES:
        groups.setdefault("n%d%s-%s" % (c.logn, "" if c.root_power == 1 else "-w%d" % c.root_power, c.direction), []).append(c)
    return list(groups.items())


def site_of(case):
    return [s for s in sites_of(case.logn, case.direction) if (s.pass_index, s.stage) == (case.pass_index, case.stage)][0]


# ------------------------------------------------------------------------------------------------ the emulation
EVENTS = ("lazy_ge_p", "lazy_wrap", "lazy_wrap_ge_p", "lazy_first_ge_p", "sub_minuend_ge_p", "sub_borrow", "mul_operand_ge_p",
          "canon_ge_p", "add_wrap", "add_ge_p")                # csrc/gl.hpp: GL_EV_*
OFF, PLANT, RECORD = 0, 1, 2
_EMU = []


def emulation():
    """tests/emu/libbfs_emu.so, built the way the host tests build it"""
    if not _EMU:
        if EMU_DIR not in sys.path:
            sys.path.insert(0, EMU_DIR)
        from build_emu import build_emulation
        lib = ctypes.CDLL(build_emulation())
        lib.emu_gl_ntt.argtypes = [vp, u64, u64, vp, u64, u32, u32, u64, u64, u64]
        lib.emu_canonical_violations.argtypes = [ctypes.c_int]
        lib.emu_canonical_violations.restype = ctypes.c_ulonglong
        lib.emu_site_control.argtypes = [ctypes.c_int, u32, u32, vp, u64]
        lib.emu_site_control.restype = None
        lib.emu_site_words.argtypes = [vp]
        lib.emu_site_words.restype = ctypes.c_ulonglong
        lib.emu_site_events.argtypes = [ctypes.c_int, vp, vp]
        lib.emu_schedule.argtypes = [u32, u64, u64, ctypes.c_int, ctypes.c_int, vp, vp]
        lib.emu_set_schedule.argtypes = [ctypes.c_int, u32, u64]
        slots = ctypes.c_int()
        assert lib.emu_site_events(0, None, ctypes.byref(slots)) == len(EVENTS)
        lib.site_slots = slots.value
        _EMU.append(lib)
    return _EMU[0]


def slot_of(pass_index, stage):
    return 1 + 3 * pass_index + (stage - 1)


def planned_instances(lib, oracle, logn):
    """{(mode, S, schedule)} of the steps the planner schedules for a full-size 2^logn transform"""
    root = oracle.primitive_nth_root(1 << logn)
    raw, virtual = (u64 * 32)(), u32()
    count = lib.emu_schedule(logn, 1 << logn, root, 0, 1, raw, ctypes.byref(virtual))
    assert count >= 1 and virtual.value == 0
    sched = lib.emu_set_schedule(-1, logn, root)
    return {(int(raw[8 * k + 1]), int(raw[8 * k + 2]), sched) for k in range(count)}


def call_of(oracle, case):
    """(root, shift, post_scale) of the case's bfs_gl_ntt / emu_gl_ntt call, and w"""
    n = 1 << case.logn
    w = oracle.power(oracle.primitive_nth_root(n), case.root_power)
    if case.direction == "inverse":
        return (oracle.inv(w), 1, oracle.inv(n)), w
    return (w, COSET_SHIFT if case.direction == "coset" else 1, 1), w


def emulate(lib, case, call, x, mode=OFF, site_buffer=None):
    """one emulated call on the case's columns -> (output, words planted / recorded, overrun, violations, events[slot][event])"""
    n, batch = 1 << case.logn, case.batch
    x = np.ascontiguousarray(x, dtype=np.uint64)
    assert x.size == n * batch
    out = np.zeros(n * batch, dtype=np.uint64)
    events = np.zeros((lib.site_slots, len(EVENTS)), dtype=np.uint64)
    lib.emu_canonical_violations(1)
    lib.emu_site_events(1, None, None)
    if mode != OFF:
        assert site_buffer.dtype == np.uint64 and site_buffer.flags["C_CONTIGUOUS"]
        lib.emu_site_control(mode, case.pass_index, case.stage, site_buffer.ctypes.data, site_buffer.size)
    try:
        rc = lib.emu_gl_ntt(x.ctypes.data, n, n, out.ctypes.data, n, case.logn, batch, call[0], call[1], call[2])
        overrun = ctypes.c_ulonglong()
        words = lib.emu_site_words(ctypes.byref(overrun))
    finally:
        lib.emu_site_control(OFF, 0, 0, None, 0)
    assert rc == 0, rc
    violations = lib.emu_canonical_violations(1)
    lib.emu_site_events(1, events.ctypes.data, None)
    return out, int(words), int(overrun.value), int(violations), events


Built = collections.namedtuple("Built", "case call V x want")


def expected_output(oracle, case, x):
    """the oracle's transform of the case's columns x -- the expected output of the call, from x alone"""
    n = 1 << case.logn
    _, w = call_of(oracle, case)
    want = []
    for b in range(case.batch):
        col = x[b * n:(b + 1) * n]
        if case.direction == "forward":
            want.append(oracle.ntt(w, col))
        elif case.direction == "inverse":
            want.append(oracle.intt(w, col))
        else:
            want.append(oracle.fast_coset_evaluate(col, COSET_SHIFT, w, n))
    return np.concatenate(want)


def build_case(oracle, case, lib=None, inputs_dir=None):
    """-> Built: the call, the planted site vector, the input that produces it and the oracle's output for that input
    (x and want hold the case's columns one after the other, n words each).
    inputs_dir: a directory where the inputs are kept from one build to the next (a test module and its child processes share one):
    a case whose x is there is not built again -- V is then None --, and a case that is built leaves its x there."""
    n, batch = 1 << case.logn, case.batch
    call, w = call_of(oracle, case)
    kept = os.path.join(inputs_dir, case_id(case) + ".npy") if inputs_dir else None
    if kept and os.path.exists(kept):
        x = np.load(kept)
        assert x.dtype == np.uint64 and x.shape == (n * batch,)
        return Built(case, call, None, x, expected_output(oracle, case, x))
    lib = lib or emulation()
    # (the draw depends on the whole case, so that no two sites see the same vector)
    key = [case.seed, case.logn, case.root_power, DIRECTIONS.index(case.direction), case.pass_index, case.stage]
    V = np.concatenate([site_vector(n, key + [b]) for b in range(batch)])
    y, words, overrun, _, _ = emulate(lib, case, call, np.zeros(n * batch, dtype=np.uint64), PLANT, V)
    assert words == n * batch and overrun == 0, "the plant must consume exactly n words per column: %d of %d, %d beyond" % (words, n * batch, overrun)
    x = []
    for b in range(batch):
        col = y[b * n:(b + 1) * n]
        if case.direction == "forward":
            x.append(oracle.intt(w, col))
        elif case.direction == "inverse":
            x.append(oracle.ntt(w, col))
        else:
            x.append(oracle.fast_coset_interpolate(COSET_SHIFT, w, col))
    x = np.concatenate(x)
    if kept:
        np.save(kept + ".part.npy", x)
        os.replace(kept + ".part.npy", kept)
    return Built(case, call, V, x, expected_output(oracle, case, x))


def required_events(site):
    """the classes of operands that must occur AT the site (tests/test_ntt_planted_host.py): where the butterflies keep unreduced sums,
    every branch of gl_add_lazy, a minuend >= p and an unreduced value >= p met by what consumes it there -- gl_canon where the unit
    twiddle's register is reduced, else the site's own products; where they keep none, both reductions of gl_add and a borrow"""
    if not site.lazy:
        return ("add_wrap", "add_ge_p", "sub_borrow")
    need = ["lazy_ge_p", "lazy_wrap", "lazy_first_ge_p", "sub_minuend_ge_p"]
    if site.radix_bits >= 2:
        need.append("lazy_wrap_ge_p")       # (a sum that wraps and is still >= p needs a first operand > p: a second level, radix >= 4)
    if site.canon:
        need.append("canon_ge_p")
    elif site.multiplies:
        need.append("mul_operand_ge_p")
    return tuple(need)


def check_case(lib, built):
    """the recording run on x -> (reached, output_ok, violations, {event: count at the site}, mul_operand_ge_p over the whole run)"""
    case = built.case
    rec = np.zeros_like(built.V)
    out, words, overrun, violations, events = emulate(lib, case, built.call, built.x, RECORD, rec)
    reached = words == rec.size and overrun == 0 and bool((rec == built.V).all())
    at = events[slot_of(case.pass_index, case.stage)]
    return reached, bool((out == built.want).all()), violations, {e: int(at[k]) for k, e in enumerate(EVENTS)}, int(events[:, EVENTS.index("mul_operand_ge_p")].sum())


def find_seed(oracle, case, tries=64):
    """the first seed from 1 on with which every required class occurs at the site (how SEEDS was filled)"""
    lib = emulation()
    need = required_events(site_of(case))
    for seed in range(1, tries + 1):
        _, _, _, at, mul_total = check_case(lib, build_case(oracle, case._replace(seed=seed), lib))
        if all(at[e] for e in need) and (mul_total or not site_of(case).lazy):
            return seed
    return None


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from oracle import ref_oracle
    for c in CASES:
        s = find_seed(ref_oracle, c)
        if s != 1:
            print('    "%s": %s,' % (case_id(c), s), flush=True)
