"""The checker of tests/pointwise_check.py on synthetic codewords, without a GPU: a small program's trace is padded and extended on
the host, every column is interpolated and randomised the way the prover does it (f = INTT(column) + c (X^h - 1)) and evaluated on
the FRI domain with the oracle (oracle.fast_coset_evaluate).  The quotients and the combination are then the checker's own formulas
at every row -- so the pointwise half agrees by construction, and what this shows is that
  * the formulas describe the real protocol: from a trace that satisfies the AIR they give codewords of exactly the degrees the
    prover's symbolic bounds promise (a wrong zerofier, a wrong neighbour row or a wrong term order would not be low-degree), and
  * each kind of fault is caught: a word changed at a row the pointwise half does not sample (degree), a whole quotient scaled by a
    constant (pointwise), a value stored as v + p (canonical), a wrong degree shift in the combination (pointwise)."""
import numpy as np
import pytest

import pointwise_check as pc
from pointwise_check import P


@pytest.fixture(scope="module")
def synthetic(oracle):
    from stark_brainfuck_amd import air
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    from stark_brainfuck_amd.vm import VirtualMachine
    program = VirtualMachine.compile(",[++.,]")
    running_time, inputs, outputs = VirtualMachine.run(program, input_data=list("abc\x00"))
    matrices = VirtualMachine.simulate(program, input_data=list(inputs))
    stark = BrainfuckStark(running_time, len(matrices[1]), program, inputs, outputs)
    rng = np.random.default_rng(11)

    def sample(k):
        return [tuple(int(v) for v in rng.integers(1, P, 3, dtype=np.uint64)) for _ in range(k)]
    challenges, initials = sample(11), sample(2)
    for table, matrix in zip(stark.tables, (matrices[0], matrices[2], matrices[1], matrices[3], matrices[4])):
        table.matrix = matrix
        table.pad()
        table.extend(challenges, initials)
    terminals = stark.get_terminals()
    n, offset, omega = stark.fri.domain.length, stark.fri.domain.offset.value, stark.fri.domain.omega.value

    def low_degree_extension(column, table):
        """the randomised interpolant of one trace column (table.py:112-136: one extra point, f = f0 + c (X^h - 1)) on the domain"""
        h = table.height
        coeffs = np.zeros(h + 1, dtype=np.uint64)
        coeffs[:h] = oracle.intt(table.omicron.value, column)
        if table.num_randomizers:
            c = int(rng.integers(1, P, dtype=np.uint64))
            coeffs[0], coeffs[h] = oracle.sub(int(coeffs[0]), c), c
        return oracle.fast_coset_evaluate(coeffs, offset, omega, n)
    base, ext = [], []
    for t in stark.tables:
        assert t.height > 0
        columns = t.base_array()
        base.append(np.stack([low_degree_extension(columns[c], t) for c in range(t.base_width)]))
        ext.append(np.stack([np.stack([low_degree_extension(col[limb], t) for limb in range(3)]) for col in t.ext_columns]))
    randomizer = np.stack([oracle.fast_coset_evaluate(rng.integers(0, P, stark.max_degree + 1, dtype=np.uint64), offset, omega, n)
                           for _ in range(3)])
    bounds = [b for t in stark.tables for b in t.all_quotient_degree_bounds(challenges, terminals)]
    bounds += [a.quotient_degree_bound() for a in stark.permutation_arguments]
    spec = pc.PointwiseSpec(stark, challenges, terminals, bounds, b"synthetic weights seed")
    # the "prover": the checker's formulas at every row of the domain
    full = pc.Checker(spec, base, ext, randomizer, range(n))
    quotients = np.array([full.expected[i] for i in range(n)], dtype=np.uint64).transpose(1, 2, 0)      # (quotients, 3, n)
    combination = np.array([spec.combination_at(i, full.values, tuple(int(v) for v in randomizer[:, i]), full.expected[i])
                            for i in range(n)], dtype=np.uint64).T
    rows = pc.sample_rows(n, spec.unit_distances(), count=64, seed=3)
    checker = pc.Checker(spec, base, ext, randomizer, rows)
    assert air.X0 not in [tuple(c) for c in challenges]
    return dict(stark=stark, spec=spec, checker=checker, quotients=quotients, combination=combination, rows=rows, n=n,
                base=base, ext=ext, randomizer=randomizer)


def kinds(failures):
    return {kind for kind, _ in failures}


def test_checker_accepts_codewords_of_a_trace_that_satisfies_the_air(synthetic):
    s = synthetic
    checker, spec = s["checker"], s["spec"]
    assert s["n"] == 1 << 11 and len(s["rows"]) < s["n"] // 4
    assert checker.inputs() == []
    for q in range(len(spec.labels)):
        assert checker.quotient(q, s["quotients"][q]) == [], spec.labels[q]
    assert checker.combination(s["combination"]) == []
    # the bounds are tight: most quotients reach theirs, so a checker one degree too strict would have failed above
    tight = [q for q in range(len(spec.labels)) if pc.degree(s["quotients"][q], spec.omega) == spec.quotient_degree_bounds[q]]
    assert len(tight) > len(spec.labels) // 2


def test_a_word_changed_at_an_unsampled_row_breaks_the_degree(synthetic):
    s = synthetic
    checker, n = s["checker"], s["n"]
    row = next(i for i in range(n // 3, n) if i not in set(s["rows"]))
    for q in (0, len(s["spec"].labels) - 1):                   # a processor boundary quotient, a difference quotient
        bad = s["quotients"][q].copy()
        bad[1, row] = (int(bad[1, row]) + 1) % P
        assert kinds(checker.quotient(q, bad)) == {"degree"}
    bad = s["combination"].copy()
    bad[0, row] = (int(bad[0, row]) + 12345) % P
    assert kinds(checker.combination(bad)) == {"degree"}
    bad = [e.copy() for e in s["ext"]]
    bad[2][0, 2, row] ^= 1
    assert kinds(pc.Checker(s["spec"], s["base"], bad, s["randomizer"], s["rows"]).inputs()) == {"degree"}


def test_a_quotient_scaled_by_a_constant_is_caught_pointwise(synthetic):
    s = synthetic
    checker, spec = s["checker"], s["spec"]
    nonzero = [q for q in range(len(spec.labels)) if s["quotients"][q].any()]       # (some constraints vanish identically here)
    assert len(nonzero) > len(spec.labels) // 2
    for q in nonzero[::5] + nonzero[-2:]:
        bad = np.stack([pc.oracle.hadamard(plane, np.full(s["n"], 3, dtype=np.uint64)) for plane in s["quotients"][q]])
        failures = checker.quotient(q, bad)
        assert "pointwise" in kinds(failures), spec.labels[q]
        assert spec.labels[q][0] in failures[0][1]


def test_a_value_stored_as_v_plus_p_is_caught(synthetic):
    s = synthetic
    checker = s["checker"]
    q = next(q for q in range(len(s["spec"].labels)) if (s["quotients"][q] < (1 << 32) - 1).any())
    bad = s["quotients"][q].copy()
    limb, row = [int(v[0]) for v in np.nonzero(bad < (1 << 32) - 1)]
    bad[limb, row] += np.uint64(P)
    assert kinds(checker.quotient(q, bad)) == {"canonical"}
    bad = s["randomizer"].copy()
    bad[0, 5] = np.uint64(P)
    assert kinds(pc.Checker(s["spec"], s["base"], s["ext"], bad, s["rows"]).inputs()) == {"canonical"}


def test_a_wrong_degree_shift_is_caught_pointwise(synthetic):
    s = synthetic
    spec = s["spec"]
    other = pc.PointwiseSpec(s["stark"], spec.challenges, spec.terminals, spec.quotient_degree_bounds, b"synthetic weights seed",
                             shift_tweak=lambda shifts: shifts + (np.arange(len(shifts), dtype=np.uint64) == 20).astype(np.uint64))
    checker = pc.Checker(other, s["base"], s["ext"], s["randomizer"], s["rows"])
    assert "pointwise" in kinds(checker.combination(s["combination"], check_degree=False))


def test_sampled_rows_cover_the_edges():
    rows = set(pc.sample_rows(1 << 22, [0, 64, 32], count=1024, seed=0))
    assert {0, 1, 2, (1 << 21) - 1, 1 << 21, (1 << 21) + 1, (1 << 22) - 1, 63, 64, (1 << 22) - 64, (1 << 22) - 63} <= rows
    assert {(1 << 20) - 1, 1 << 20, (1 << 20) + 1, 255, 256, 257} <= rows
    assert len(rows) >= 1024 + 30 and max(rows) < 1 << 22


def test_degree_of_folded_codewords(oracle):
    n, offset = 1 << 10, 7
    omega = oracle.primitive_nth_root(n)
    rng = np.random.default_rng(5)
    planes = np.stack([oracle.fast_coset_evaluate(rng.integers(0, P, d + 1, dtype=np.uint64), offset, omega, n) for d in (100, 300, 37)])
    assert pc.degree(planes[1], omega) == 300 and pc.degree(planes, omega) == 300
    assert pc.degree(np.zeros(n, dtype=np.uint64), omega) == -1
    planes[2, 17] = (int(planes[2, 17]) + 1) % P
    assert pc.degree(planes, omega) == n - 1
