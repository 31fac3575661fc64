"""The carry-chain models of tests/field_states.py against plain modular arithmetic, and the coverage of the operand sets the GPU
tests feed to the kernels: every REQUIRED state is reached, and every other state is either witnessed (and then required) or listed in
the helper's "no witness found" table with the search that was tried."""
import random

import field_states as fs

P = fs.P


def test_product_models_equal_the_plain_product():
    pairs = fs.fused_operands() + fs.random_pairs(100000, seed=1)
    for a, b in pairs:
        want = a * b % P
        assert fs.fused_product(a, b)[0] == want, (hex(a), hex(b))
        lazy = fs.lazy_product(a, b)[0]
        assert 0 <= lazy < 1 << 64 and lazy % P == want, (hex(a), hex(b))


def test_fold_model_is_canonical_for_every_64_bit_base():
    rng = random.Random(2)
    edges = (0, 1, fs.EPS, 1 << 32, P - 1, P, P + 1, fs.M64 - fs.EPS, fs.M64)
    operands = [(w, base) for w in (0, 1, 2, fs.M32 - 1, fs.M32) for base in edges]
    operands += [(rng.randrange(1 << 32), rng.randrange(1 << 64)) for _ in range(100000)]
    operands += [(rng.randrange(1 << rng.randrange(1, 33)), fs.M64 - rng.randrange(1 << 34)) for _ in range(20000)]
    for w, base in operands:
        assert fs.fold_word(w, base)[0] == (base + (w << 64)) % P, (w, hex(base))
    # Cf and Kf cannot both be set: a wrapped sum is below w * (2^32 - 1)
    assert fs.fold_states(operands) == {(0, 0), (0, 1), (1, 0)}


def test_sum_model_equals_the_plain_sum():
    rng = random.Random(3)
    sums = fs.accumulator_witness_sums() + fs.palette_sums(2000, 19, seed=4)
    sums += [[(rng.randrange(P), rng.randrange(P)) for _ in range(rng.randrange(1, 20))] for _ in range(100000 // 10)]
    for pairs in sums:
        assert fs.lazy_sum(pairs)[0] == sum(a * b for a, b in pairs) % P, pairs


def test_fused_product_operands_reach_the_required_states():
    reached = fs.fused_states(fs.fused_operands())
    assert fs.FUSED_REQUIRED <= reached, sorted(fs.FUSED_REQUIRED - reached)


def test_every_other_fused_state_is_witnessed_or_listed():
    """the floor holds what has a witness; a state outside it is either reached by the exported operands (then it belongs in
    FUSED_REQUIRED) or stands in FUSED_NO_WITNESS"""
    reached = fs.fused_states(fs.fused_operands())
    assert reached <= fs.FUSED_REQUIRED, "witnessed but not required: %s" % sorted(reached - fs.FUSED_REQUIRED)
    every = {(k, b, c, cf, kf) for k in (0, 1) for b in (0, 1) for c in (0, 1) for cf in (0, 1) for kf in (0, 1)}
    assert every - fs.FUSED_REQUIRED == set(fs.FUSED_NO_WITNESS), sorted((every - fs.FUSED_REQUIRED) ^ set(fs.FUSED_NO_WITNESS))
    # the search behind that table, run again (a slice of it: the table names the full one)
    assert set(fs.fused_search(tries=20000)) <= fs.FUSED_REQUIRED


def test_planted_launches_reach_the_required_accumulator_states():
    """the launches tests/test_gpu_pointwise_edges.py plants, modelled from the operand streams of csrc/lazy.hpp"""
    acc, inner = set(), set()
    for table in range(5):
        for launch in fs.planted_launches(table, fs.PLANTED_ROWS):
            a, r = fs.launch_states(launch, fs.PLANTED_ROWS)
            acc |= a
            inner |= r
    assert fs.ACC_REQUIRED <= acc, sorted(fs.ACC_REQUIRED - acc)
    assert fs.ACC_INNER_REQUIRED <= inner, sorted(fs.ACC_INNER_REQUIRED - inner)
    assert acc <= fs.ACC_REQUIRED, "witnessed but not required: %s" % sorted(acc - fs.ACC_REQUIRED)
    assert inner <= fs.ACC_INNER_REQUIRED, "witnessed but not required: %s" % sorted(inner - fs.ACC_INNER_REQUIRED)
    every_acc = {(a, b, c, d, e) for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1) for e in (0, 1)}
    every_inner = {(a, b, c, d) for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1)}
    assert every_acc - fs.ACC_REQUIRED == set(fs.ACC_NO_WITNESS)
    assert every_inner - fs.ACC_INNER_REQUIRED == set(fs.ACC_INNER_NO_WITNESS)


def test_planted_seeds_are_what_the_search_returns():
    """the recorded launch seeds of the two smallest tables are the greedy search's own answer"""
    for table in (3, 4):
        kept, _, _ = fs.planted_search(table, fs.PLANTED_ROWS, tries=fs.PLANTED_TRIES)
        assert tuple(kept) == fs.PLANTED_SEEDS[table], (table, kept)


def test_witness_sums_are_in_the_states_they_are_named_for():
    for state, pairs in fs.ACC_WITNESSES.items():
        assert fs.lazy_sum(pairs)[1][0] == state, state
    for state, pairs in fs.ACC_INNER_WITNESSES.items():
        assert fs.lazy_sum(pairs)[1][1] == state, state


def test_selftest_reference_is_canonical():
    for a, b in fs.fused_operands()[:300]:
        out = fs.selftest_reference(a, b)
        assert len(out) == fs.SELFTEST_OPS and all(0 <= v < P for v in out)
        assert out[2] == a * b % P and out[40] == out[2] and out[34] == out[1]
