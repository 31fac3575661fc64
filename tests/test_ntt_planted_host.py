"""CPU checks of the planted NTT cases (tests/ntt_planted.py) on the host emulation of the tile kernels: for every case the input
really puts the chosen operands at the chosen site, the emulated output is the oracle's, no operand that must be canonical is not, and
the operands reach every class of the site's arithmetic that they are there for -- the event counters of csrc/gl.hpp
(-DBFS_CHECK_CANONICAL), per site.  The emulation computes with 128-bit integers; the device's instruction sequences meet the same
inputs in tests/test_gpu_ntt_planted.py.  Each test prints its counts (pytest -s shows the table)."""
import ctypes

import pytest

import ntt_planted as planted
from field_states import PALETTE, P


@pytest.fixture(scope="module")
def emu():
    return planted.emulation()


@pytest.mark.parametrize("case", planted.CASES, ids=planted.CASE_IDS)
def test_planted_operands_reach_their_site(emu, oracle, case):
    """The recording run on x returns V word for word at the site; the emulated output equals the oracle's; no canonical-operand
    violation; and at the site itself:
      butterflies that keep unreduced sums (OUT_LAZY): every branch of gl_add_lazy (>= p without wrap, wrapped, wrapped and still >= p
        after + EPS -- radix >= 4 only, it needs a first operand > p, which only a second level has --, first operand >= p), a gl_sub
        minuend >= p, and an unreduced value >= p in what consumes it there: gl_canon where the site runs it (the unit-twiddle register
        of a stage 1; not when n^-1 is folded into that twiddle, and never at a stage 2), else the site's own products; over the whole
        run a gl_mul operand >= p (a first pass' unreduced store is consumed by the next pass' load);
      the others: both reductions of gl_add (wrapped; >= p without wrap) and a gl_sub borrow."""
    site = planted.site_of(case)
    built = planted.build_case(oracle, case, emu)
    assert (built.V < P).all() and (built.x < P).all() and (built.want < P).all()
    reached, output_ok, violations, at, mul_total = planted.check_case(emu, built)
    need = planted.required_events(site)
    print("%-24s %-5s violations %d  %s  mul_operand_ge_p(run) %d" % (planted.case_id(case), "lazy" if site.lazy else "plain", violations,
                                                                   "  ".join("%s %d" % (e, at[e]) for e in need), mul_total))
    assert reached, "the input does not put the planted vector at the site"
    assert output_ok, "the emulated output differs from the oracle's"
    assert violations == 0
    assert all(at[e] >= 1 for e in need), {e: at[e] for e in need}
    if site.lazy:
        assert mul_total >= 1


def test_the_cases_cover_the_planners_instances(emu, oracle):
    """emu_schedule over log n = 4 .. 20 yields exactly the (mode, S, schedule) instances the case list claims to reach, size by size,
    and every site of every size has a case in each direction"""
    every = set()
    for logn in range(4, 21):
        got = planted.planned_instances(emu, oracle, logn)
        assert got == planted.claimed_instances(logn), (logn, sorted(got))
        every |= got
    S, F, C = planted.SINGLE, planted.FIRST, planted.COLUMN
    assert every == ({(S, s, 0) for s in range(4, 13)} | {(F, 7, 0), (F, 8, 0), (C, 6, 0), (C, 7, 0), (C, 8, 0)} |      # one and two passes
                     {(F, 6, 0), (C, 5, 0)} |                                                                           # 2^17, chain
                     {(F, 6, 1), (F, 7, 1), (C, 6, 1), (C, 7, 1)})                                                      # 2^18 .. 2^20, balanced
    have = {(c.logn, c.direction, c.pass_index, c.stage) for c in planted.CASES if c.root_power == 1}
    for logn in planted.PLAN:
        for direction in planted.DIRECTIONS:
            for s in planted.sites_of(logn, direction):
                assert (logn, direction, s.pass_index, s.stage) in have


def test_the_other_root_moves_the_unit_twiddle(emu, oracle):
    """the 2^13 cases with the root w^3: another u^-1 mod 16, so another register of the radix-16 stages holds output digit 0"""
    emu.emu_plan.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    uinv = []
    for power in (1, 3):
        npass, u = ctypes.c_uint32(), ctypes.c_uint32()
        bits, logc = (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * 4)()
        root = oracle.power(oracle.primitive_nth_root(1 << 13), power)
        assert emu.emu_plan(13, root, ctypes.byref(npass), bits, logc, ctypes.byref(u)) == 0
        uinv.append(u.value)
    assert uinv[0] != uinv[1], uinv
    assert any(c.root_power == 3 and c.logn == 13 for c in planted.CASES)


def test_the_palette():
    """PALETTE and its negatives, with 2^32 +- 1, p - 2^32 and 2^63 +- 1; canonical; the sub-palettes draw from it"""
    for v in PALETTE:
        assert v in planted.VALUES and (P - v) % P in planted.VALUES
    for v in ((1 << 32) - 1, (1 << 32) + 1, P - (1 << 32), (1 << 63) - 1, (1 << 63) + 1):
        assert v in planted.VALUES
    assert all(0 <= v < P for v in planted.VALUES)
    V = planted.site_vector(4096, [1, 2, 3])
    assert set(int(v) for v in V) <= set(planted.VALUES)
    assert (V == planted.site_vector(4096, [1, 2, 3])).all() and (V != planted.site_vector(4096, [1, 2, 4])).any()
