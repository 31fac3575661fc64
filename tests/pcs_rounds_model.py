"""A CPython model of openings across commitments (stark_brainfuck_amd/pcs.py: open_rounds / verify_rounds; include/bfstark_rounds.h)
for tests/test_pcs_rounds_host.py and tests/test_gpu_pcs_rounds.py: built on tests/pcs_model.py and tests/pcs_groups_model.py and,
through them, on the oracle's NTT and the FRI models, all imported unchanged.  The package is never imported here.

Statement.  R <= 4 commitments C_0 .. C_{R-1} over the same domain, made at any moments of ONE transcript (each `commit` pushes its root;
the caller pushes, pulls and draws challenges in between).  Their row columns are numbered through: column c of C_r is global column
first[r] + c, first[r] = m_0 + .. + m_{r-1}.  A plan over the global columns is tests/pcs_groups_model.py's Plan, and the quotient is its
formula word for word over the rows laid one behind the other.
Protocol, where `open` begins (all roots are in the stream already): the distinct points in order of first appearance (a list of
elements); the shape (tuple(widths), [(tuple(columns_g), tuple(point indices)) per group]) of plain ints; the values, a list per group of
a list per point of a list per column; lambda; the root of the tree over g (of the coset tree when the FRI mode commits to cosets);
t indices; per index i: for r = 0 .. R-1 the row tuple of C_r at x_i and its path, then the opening of g; FRI over g.

The split of the quotient between kernel launches (csrc/deep_core.hpp: deep_rounds_split) is restated in `launches` below: the tests
hold the emulation's and the library's launch counts against it.
"""
import numpy as np

import fri_coset_model
import fri_grinding_model
import pcs_groups_model as gmodel
import pcs_model as model

P = model.P
LAUNCH_COLUMNS, LAUNCH_GROUPS, LAUNCH_PAIRS, LAUNCH_POINTS = 32, 8, 16, 8


def launches(plan):
    """the rule, restated: groups in plan order; a launch takes groups while its columns <= 32, its groups <= 8, its pairs <= 16 and
    the distinct points among its groups <= 8; the first group that would break one of these starts the next launch.
    -> per launch the list of the plan's group numbers"""
    plan = plan if isinstance(plan, gmodel.Plan) else gmodel.Plan(plan)
    out, columns, pairs, points = [[]], 0, 0, set()
    for g, (group, indices) in enumerate(plan.groups):
        assert len(group) <= LAUNCH_COLUMNS and len(indices) <= 4
        if out[-1] and (columns + len(group) > LAUNCH_COLUMNS or len(out[-1]) + 1 > LAUNCH_GROUPS or pairs + len(indices) > LAUNCH_PAIRS
                        or len(points | set(indices)) > LAUNCH_POINTS):
            out.append([])
            columns, pairs, points = 0, 0, set()
        out[-1].append(g)
        columns, pairs, points = columns + len(group), pairs + len(indices), points | set(indices)
    return out


def first_columns(widths):
    return [sum(widths[:r]) for r in range(len(widths))]


def global_column(widths, r, c):
    assert 0 <= r < len(widths) and 0 <= c < widths[r]
    return first_columns(widths)[r] + c


def commit(o, ext_polys, base_polys, N, offset, omega, proof_stream):
    """one round: tests/pcs_model.py's commit on the transcript the rounds share; pushes the root"""
    return model.commit(o, ext_polys, base_polys, N, offset, omega, proof_stream=proof_stream)


def widths_of(commitments):
    return [len(c["ext"]) + len(c["base"]) for c in commitments]


def codewords(commitments):
    """the codewords of all commitments in global column order"""
    return [cw for c in commitments for cw in c["codewords"]]


def true_values(commitments, plan):
    polys = []
    for c in commitments:
        polys += [(True, f) for f in c["ext"]] + [(False, f) for f in c["base"]]

    def at(column, z):
        is_ext, f = polys[column]
        return model.evaluate_ext(f, z) if is_ext else model.evaluate_base(f, z)
    return [[[at(c, plan.points[p]) for c in columns] for p in indices] for columns, indices in plan.groups]


def open(o, commitments, plan, offset, omega, expansion, t, folding_factor=2, coset_leaves=False, grinding_bits=0, forced_values=None):
    """commitments: what `commit` returned, in the order of the numbering, all on one proof stream
    -> dict(values, lam, g, g_root, indices, fri, proof_stream, bytes, plan, widths, start: the stream's length where the opening began)"""
    ps, N = commitments[0]["proof_stream"], commitments[0]["N"]
    assert all(c["proof_stream"] is ps and c["N"] == N for c in commitments) and 1 <= len(commitments) <= 4
    plan = plan if isinstance(plan, gmodel.Plan) else gmodel.Plan(plan)
    widths = widths_of(commitments)
    assert plan.m == sum(widths) and not any(model.in_domain(z, N, offset) for z in plan.points)
    start = len(ps.objects)
    ps.push([o.make_xfe(z) for z in plan.points])
    ps.push((tuple(widths), plan.shape))
    values = true_values(commitments, plan) if forced_values is None else forced_values
    ps.push([[[o.make_xfe(v) for v in per_point] for per_point in per_group] for per_group in values])
    lam = tuple(int(v) for v in o.xsample(ps.prover_fiat_shamir()))
    g = gmodel.quotient(codewords(commitments), N, offset, omega, plan, gmodel.combined_values(plan, values, lam), lam)
    a = folding_factor if coset_leaves else 1
    q = N // a
    if coset_leaves:
        tree, leaves, _ = fri_coset_model.coset_merkle(o, g, a)
    else:
        tree, leaves = o.xfe_merkle(g)
    ps.push(tree.root())
    indices = model.sample_indices(t, ps.prover_fiat_shamir(), N)
    for i in indices:
        for c in commitments:
            ps.push(c["rows"][i])
            ps.push(c["tree"].open(i))
        ps.push(leaves[i % q])
        ps.push(tree.open(i % q))
    oo = o if coset_leaves else model._KnownLeafs(o, {i: leaves[i] for i in indices})
    fri = fri_grinding_model.prove(oo, g, offset, omega, expansion, t, folding_factor, coset_leaves, grinding_bits, proof_stream=ps)
    out = fri["proof_stream"]
    return {"values": values, "lam": lam, "g": g, "g_root": tree.root(), "indices": indices, "fri": fri, "proof_stream": out,
            "bytes": out.serialize(), "plan": plan, "widths": widths, "start": start}


def verify(o, objects, start, roots, widths, plan, values, N, offset, omega, t, folding_factor, coset_leaves, fri_verify):
    """objects: the WHOLE stream's objects; start: the read position where the opening begins (the roots in front of it are the
    caller's to read: `roots` is what it read).  fri_verify(objects, read_index, g_root) -> bool judges what lies behind the openings.
    -> (verdict, reason)"""
    ps = o.ProofStreamOracle()
    ps.objects = list(objects)
    at = [start]

    def pull():
        at[0] += 1
        return ps.objects[at[0] - 1]

    def fiat_shamir():
        prefix = o.ProofStreamOracle()
        prefix.objects = ps.objects[:at[0]]
        return prefix.prover_fiat_shamir()
    widths = [int(w) for w in widths]
    if len(roots) != len(widths) or not 1 <= len(widths) <= 4:
        return False, "commitments"
    try:
        plan = plan if isinstance(plan, gmodel.Plan) else gmodel.Plan(plan)
    except AssertionError:
        return False, "plan"
    if plan.m != sum(widths):
        return False, "plan"
    values = [[[tuple(int(x) for x in v) for v in per_point] for per_point in per_group] for per_group in values]
    if any(model.in_domain(z, N, offset) for z in plan.points):
        return False, "points"
    if [tuple(o.xfe_limbs(z)) for z in pull()] != plan.points:
        return False, "points"
    pushed_widths, pushed_groups = pull()
    if [int(w) for w in pushed_widths] != widths:
        return False, "widths"
    if [(tuple(columns), tuple(indices)) for columns, indices in pushed_groups] != plan.shape:
        return False, "shape"
    if [[[tuple(o.xfe_limbs(v)) for v in per_point] for per_point in per_group] for per_group in pull()] != values:
        return False, "values"
    lam = tuple(int(v) for v in o.xsample(fiat_shamir()))
    Y = gmodel.combined_values(plan, values, lam)
    g_root = pull()
    indices = model.sample_indices(t, fiat_shamir(), N)
    a = folding_factor if coset_leaves else 1
    q = N // a
    for i in indices:
        columns = []
        for root, width in zip(roots, widths):
            row, path = pull(), pull()
            if not o.merkle_verify(root, i, path, o.dumps(row)):
                return False, "row path"
            if len(row) != width:
                return False, "row"
            columns += [np.array(o.xfe_limbs(e), dtype=np.uint64).reshape(3, 1) if hasattr(e, "polynomial") else np.array([e.value], dtype=np.uint64) for e in row]
        leaf, path = pull(), pull()
        if not o.merkle_verify(g_root, i % q, path, o.dumps(leaf)):
            return False, "quotient path"
        x = offset * pow(omega, i, P) % P
        want = gmodel.quotient(columns, 1, x, 1, plan, Y, lam)
        if [int(v) for v in want[:, 0]] != [int(v) for v in o.xfe_limbs(leaf[i // q] if coset_leaves else leaf)]:
            return False, "quotient value"
    return (True, "accepted") if fri_verify(ps.objects, at[0], g_root) else (False, "fri")
