"""Proving by out-of-domain openings ("Proving by out-of-domain openings"): commitments in rounds through
pcs.PolynomialCommitment, the quotients composed into ONE polynomial H, everything opened at one drawn point z with one FRI proof.
A second protocol beside prove() / verify(), through Python stages only; the reference has no counterpart.

BrainfuckStark.prove_deep / verify_deep / deep_shape / compose_into are this module's `prove`, `verify`, `make_shape` and `compose_into`.
All four modes of the protocol -- segmented or not ("Segmented composition"), zero-knowledge or not ("Zero-knowledge openings")
-- are ONE code path over a shape -- L, S, s, n, w, fri, domain, working_domain, k, m, L0, randomizer, hiding (`make_shape`) --, which the
per-proof record carries as `p.shape`: the stages and the verifier read the shape and never ask which mode made it.  Without
zero-knowledge k = m = 0, L0 = L and there is neither a masking polynomial nor a salt: no blinding launch, no draw, the same bytes.
secret_input ("Secret input") is not a shape but a claim -- "some input gives this output" -- on the zero-knowledge shapes: the
input table stays empty, the input evaluation terminal is not sent and one weight is zero (check_secret_input .. sent_terminals below say
which).  What the stages share with prove() -- padding, the extension, the terminals' objects, the weights, the stage loop, the
random source -- is reached through the `stark` object; this module does not import brainfuck_stark."""
import ctypes
import gc
from types import SimpleNamespace

import numpy as np

from . import _lib, air, table as table_mod
from .algebra import P_GOLDILOCKS
from .arrays import BaseArray, XArray, raw_ntt
from .device import DeviceBuffer, DeviceView, current_stream
from .fri import Fri
from .ip import ProofStream
from .pcs import MAX_EXT_COLUMNS, PolynomialCommitment
from .table import lde_tables, prepare_extension
from .vm import LazyTraceMatrix, VirtualMachine

_u64 = ctypes.c_uint64


def deep_opening_plan(tables, z, segments=1, randomizer=False):
    """The one opening of prove_deep / verify_deep at the drawn point z (a limb triple), from public data alone: the tables' heights,
    widths and subgroup generators.  The columns are those of the three commitments numbered through (PolynomialCommitment.
    global_column): every table's base columns in table order, then every table's extension columns, then H -- or, in the segmented
    mode, the `segments` (1 .. 16, pcs.MAX_EXT_COLUMNS) segments H_0 .. H_{s-1} of H.
      * one group per table with rows: its base columns, then its extension columns, at [z, z * omicron] -- at [z] alone for a table of
        height 1, whose next row is its own row (omicron = 1);
      * one group of the columns of all tables without rows at [z], if there is such a table (their polynomials are zero);
      * a last group (H, or all its segments) at [z] -- with randomizer=True (the zero-knowledge mode) followed by one more column of
        the third commitment, the masking polynomial R, which the opening reads and the identity does not.
    -> namespace: groups (the plan as `open_rounds` takes it), widths (the commitments' row widths), table_group (per table the index
    of its group, None for a table without rows), empty_group (index or None), h_group"""
    randomizer = int(bool(randomizer))
    if not (type(segments) is int and 1 <= segments <= MAX_EXT_COLUMNS - randomizer):
        raise ValueError("the composition polynomial has 1 .. %d segments (got %r)" % (MAX_EXT_COLUMNS - randomizer, segments))
    z = tuple(int(v) for v in z)
    num_base = sum(t.base_width for t in tables)
    base_at, ext_at = 0, num_base
    groups, table_group, empty = [], [], []
    for t in tables:
        bw, xw = t.base_width, t.full_width - t.base_width
        columns = list(range(base_at, base_at + bw)) + list(range(ext_at, ext_at + xw))
        base_at, ext_at = base_at + bw, ext_at + xw
        if t.height == 0:
            empty += columns
            table_group.append(None)
        else:
            table_group.append(len(groups))
            groups.append((columns, [z] if t.height == 1 else [z, air.xscale(z, t.omicron.value)]))
    empty_group = None
    if empty:
        empty_group = len(groups)
        groups.append((sorted(empty), [z]))
    groups.append((list(range(ext_at, ext_at + segments + randomizer)), [z]))
    return SimpleNamespace(groups=groups, widths=(num_base, ext_at - num_base, segments + randomizer), table_group=table_group,
                           empty_group=empty_group, h_group=len(groups) - 1)


def blinded_degree_bound(stark, k):
    """max_degree as the constructor computes it -- the largest transition quotient degree bound under all-ones challenges -- for trace
    interpolants of h + k coefficients (degree h + k - 1 in the place of Table.interpolant_degree()) in every table with rows; kept per k"""
    known = stark.__dict__.setdefault("_blinded_degree_bounds", {})
    if k not in known:
        # (the constructor's own call with another interpolant degree: Table keeps the symbolic expansion under these challenges)
        ones = [air.X1] * 11
        known[k] = max([1] + [t.max_transition_degree(ones, t.height + k - 1 if t.height else None) for t in stark.tables])
    return known[k]


def make_shape(stark, segmented=False, zero_knowledge=False):
    """BrainfuckStark.deep_shape: the namespace L, S, s, n, w, fri, domain, working_domain (deep_segmented_shape's docstring defines them)
    and k, m, L0, randomizer, hiding (deep_shape's docstring; DESIGN.md, "Zero-knowledge openings"): 0, 0, L, False, False unless
    zero_knowledge"""
    if not segmented and not zero_knowledge:          # one segment on the constructor's Fri: nothing is made, nothing can be refused
        S, fri = stark.max_degree + 1, stark.fri
        return SimpleNamespace(L=S, S=S, s=1, n=fri.domain.length, w=fri.domain.length, fri=fri, domain=fri.domain, working_domain=fri.domain,
                               k=0, m=0, L0=S, randomizer=False, hiding=False)
    f, e, t = stark.field, stark.expansion_factor, stark.num_colinearity_checks
    roundup = type(stark).roundup_npo2
    k = 2 * t + 6 if zero_knowledge else 0
    S = roundup(1 + blinded_degree_bound(stark, k)) if zero_knowledge else stark.max_degree + 1
    randomizer = 1 if zero_knowledge else 0
    if segmented:
        L = roundup(max([max(table.transform_coefficients(), table.height + k if table.height else 0) for table in stark.tables] + [1]))
        S = max(S, L)
        m = t + 1 if zero_knowledge else 0
        L0 = L - m
        s = -(-S // L0) if L0 > 0 else 0
        if m > L0 or s + randomizer > MAX_EXT_COLUMNS:
            raise ValueError("the composition polynomial would have %d segments of %d coefficients, more than the %d extension columns of a "
                             "commitment" % (s, L0, MAX_EXT_COLUMNS - randomizer))
    else:
        L, L0, s, m = S, S, 1, 0
    n = e * L
    w = max(n, S)
    fri = stark.fri if not segmented and n == stark.fri.domain.length else stark._segmented_fri.get(n)
    if fri is None:
        fri = stark._segmented_fri[n] = Fri(f.generator(), f.primitive_nth_root(n), n, e, stark.num_colinearity_checks, stark.xfield,
                                            folding_factor=stark.fri.folding_factor, coset_leaves=stark.fri.coset_leaves,
                                            grinding_bits=stark.fri.grinding_bits)
    working = fri.domain if w == n else Fri.Domain(f.generator(), f.primitive_nth_root(w), w)
    return SimpleNamespace(L=L, S=S, s=s, n=n, w=w, fri=fri, domain=fri.domain, working_domain=working, k=k, m=m, L0=L0,
                           randomizer=bool(randomizer), hiding=bool(zero_knowledge))


def compose_into(stark, out, log_step, weights, challenges, terminals, domain=None):
    """BrainfuckStark.compose_into"""
    domain = stark.fri.domain if domain is None else domain
    lib, n = _lib.load(), domain.length
    assert out.n == n >> log_step and out.stride == out.n
    weights = np.ascontiguousarray(weights, dtype=np.uint64)
    as_limbs = lambda w: np.ascontiguousarray(w).reshape(-1).ctypes.data_as(ctypes.POINTER(_u64))
    at, accumulate = 0, 0
    for t in stark.tables:
        nq = t.num_quotients()
        if t.height:
            mine = np.ascontiguousarray(weights[at:at + nq])
            _lib.check(lib.bfsc_air_compose(t.table_index, t.base_codewords.ptr, t.ext_codewords.ptr, *t._domain_arguments(domain),
                                            *table_mod._air_arguments(t, challenges, terminals), as_limbs(mine), log_step, accumulate, out.ptr,
                                            current_stream()))
            accumulate = 1
        at += nq
    for j, pa in enumerate(stark.permutation_arguments):
        lt, rt = stark.tables[pa.lhs[0]], stark.tables[pa.rhs[0]]
        mine = np.ascontiguousarray(weights[at + j])
        _lib.check(lib.bfsc_difference_compose(lt.ext_codeword_ptr(pa.lhs[1]), rt.ext_codeword_ptr(pa.rhs[1]), n.bit_length() - 1, domain.offset.value,
                                               domain.omega.value, as_limbs(mine), log_step, accumulate, out.ptr, current_stream()))
        accumulate = 1


# ---- the secret input ("Secret input"): what the mode leaves out, said once for the prover, the verifier and the DEBUG check
def check_secret_input(stark, shape):
    """the two refusals of secret_input=True: a claim that states its input, and a shape that hides nothing"""
    if len(stark.input_symbols):
        raise ValueError("secret_input=True proves knowledge of an input the claim does not state: construct the object with input_symbols=\"\"")
    if not shape.hiding:
        raise ValueError("secret_input=True needs zero_knowledge=True: without it the proof would hide nothing of the input")


def _mentions_terminal(expression, index):
    stack, seen = [expression], set()
    while stack:
        e = stack.pop()
        if id(e) in seen:
            continue
        seen.add(id(e))
        if e.op == "t" and e.val == index:
            return True
        stack += [c for c in (e.a, e.b) if c is not None]
    return False


def dropped_weight(stark):
    """Which of the deep_weight_count() weights a secret-input proof replaces by zero: the position -- counted as compose_into and
    _verify_stream count, through every table's air.all() in table order -- of the one terminal constraint of the processor table
    that holds its running input evaluation against the input evaluation terminal (air.ProcessorAir.terminal: term(2) - IEV)"""
    index, at, found = stark.input_table.terminal_index, 0, []
    for t in stark.tables:
        for kind, constraints in t.air.all():
            for e in constraints:
                if t is stark.processor_table and kind == "terminal" and _mentions_terminal(e, index):
                    found.append(at)
                at += 1
    assert len(found) == 1, "the processor table has %d terminal constraints on the input evaluation terminal" % len(found)
    return found[0]


def secret_input_weights(stark, weights):
    """the sampled weights ((count, 3) uint64, or a list of triples) as a secret-input proof uses them: a copy with dropped_weight() zero"""
    at = dropped_weight(stark)
    if isinstance(weights, np.ndarray):
        weights = weights.copy()
        weights[at] = 0
    else:
        weights = list(weights)
        weights[at] = air.X0
    return weights


def sent_terminals(stark, secret_input):
    """the indices (BrainfuckStark.get_terminals) of the terminals in the stream, in its order: all five, or all but the input evaluation"""
    return [i for i in range(5) if not (secret_input and i == stark.input_table.terminal_index)]


# ---- the prover: one function per stage of (stark, p), named after the `timing` key the stage ends on, over one per-proof record `p`
def prove(stark, program, matrices, proof_stream, shape, secret_input=False):
    """BrainfuckStark.prove_deep on `shape`; matrices: processor, memory, instruction, input, output"""
    processor_matrix, memory_matrix, instruction_matrix, input_matrix, output_matrix = matrices
    assert len(processor_matrix) + len(program) == len(instruction_matrix)
    if secret_input:
        check_secret_input(stark, shape)
        # the claim's input table has no rows; the caller's input matrix is dropped here, before any stage sees it
        input_matrix = LazyTraceMatrix(np.zeros((0, stark.input_table.base_width), dtype=np.uint64), VirtualMachine.field)
    gc.freeze()          # (as prove(): the trace matrices' objects are not walked by collections during the proof)
    try:
        # domain, n: where the trace is extended to and H is computed from (the working domain); the commitments are pc's, on the shape's fri
        p = SimpleNamespace(matrices=(processor_matrix, instruction_matrix, memory_matrix, input_matrix, output_matrix), proof_stream=proof_stream,
                            domain=shape.working_domain, n=shape.w, stream=current_stream(), pc=PolynomialCommitment(shape.fri, hiding=shape.hiding),
                            commitments=[], shape=shape, secret_input=bool(secret_input))
        own = lambda stage: lambda p: stage(stark, p)
        return stark._run_stages(p, (("pad", own(_stage_pad)), ("base_lde", own(_stage_base_lde)), ("base_commit", own(_stage_base_commit)),
                                     ("extend", own(_stage_extend)), ("ext_lde", own(_stage_ext_lde)), ("ext_commit", own(_stage_ext_commit)),
                                     ("composition", own(_stage_composition)), ("composition_commit", own(_stage_composition_commit)),
                                     ("opening", own(_stage_opening)), ("serialize", stark._stage_serialize)))
    finally:
        gc.unfreeze()


def _stage_pad(stark, p):          # padding as prove()'s; no randomizer polynomial is drawn
    p.draw = stark._random_source()
    stark._pad_tables(p)


def _lde(stark, p, extension):
    """lde_tables onto the working domain with the shape's k blinding coefficients per column (none for k = 0) -> codewords,
    coefficients, stride, the per-table blinding buffers"""
    return table_mod.lde_tables_blinded(stark.tables, p.domain, extension=extension, blinding=p.shape.k or None)


def _polys(stark, coefficients, stride, extension, k=0):
    """the interpolants lde_tables left in `coefficients` as views, in table order: a table's own coefficient count each -- h + k with k
    blinding coefficients --, one zero coefficient for a table without rows"""
    polys, at = [], 0
    for t in stark.tables:
        count = max(t.transform_coefficients(), t.height + k if t.height else 0, 1)
        if extension:
            for c in range(t.full_width - t.base_width):
                polys.append(XArray(DeviceView(coefficients, (at + 3 * c) * stride, 3 * stride), count, stark.xfield, stride=stride))
            at += 3 * (t.full_width - t.base_width)
        else:
            polys += [BaseArray(DeviceView(coefficients, (at + c) * stride, stride), count, stark.field) for c in range(t.base_width)]
            at += t.base_width
    return polys


def _commit_codewords(p, codewords, rows):
    """the `rows` codewords (or limb planes) a commitment is made to: `codewords` as lde_tables wrote them -- unless the working
    domain is longer than the commitment domain: then every (w / n)-th word of each, gathered by one launch"""
    n, w = p.shape.n, p.shape.w
    if w == n:
        return codewords
    out = DeviceBuffer(rows * n)
    _lib.check(_lib.load().bfsg_decimate_rows(codewords.ptr, w, (w // n).bit_length() - 1, out.ptr, n, n, rows, p.stream))
    return out


def _stage_base_lde(stark, p):
    p.base_codewords, p.base_coefficients, p.base_stride, p.base_blinding = _lde(stark, p, False)
    p.base_polys = _polys(stark, p.base_coefficients, p.base_stride, False, p.shape.k)
    p.prepared_extension = prepare_extension(stark.tables)


def _stage_base_commit(stark, p):          # C0: the codewords as lde_tables wrote them are the commitment's rows
    p.base_committed = _commit_codewords(p, p.base_codewords, len(p.base_polys))
    p.commitments.append(p.pc.commit_evaluated(p.base_polys, p.base_committed, p.proof_stream))


def _stage_extend(stark, p):
    """prove()'s stage -- challenges, initials, extension, the five terminals, the trace against the AIR where check_air is set (the
    processor's running input evaluation against its own last value).  Behind it a secret-input proof forgets the input evaluation
    terminal: the slot holds zero from here on, in the kernels' terminal vector as in the verifier's"""
    stark._stage_extend(p)
    if p.secret_input:
        p.terminals[stark.input_table.terminal_index] = air.X0


def _stage_ext_lde(stark, p):
    p.ext_codewords, p.ext_coefficients, p.ext_stride, p.ext_blinding = _lde(stark, p, True)
    p.ext_polys = _polys(stark, p.ext_coefficients, p.ext_stride, True, p.shape.k)


def _stage_ext_commit(stark, p):          # C1
    p.ext_committed = _commit_codewords(p, p.ext_codewords, 3 * len(p.ext_polys))
    p.commitments.append(p.pc.commit_evaluated(p.ext_polys, p.ext_committed, p.proof_stream))


def _stage_composition(stark, p):
    """terminals, weights, H on the S points offset * omega^(k w / S) of the working domain, and its S coefficients: a coset inverse
    transform of length S with root omega^(w / S) and the domain's offset"""
    from . import debug_checks
    terminal_objects = stark._terminal_objects(p.terminals)
    for i in sent_terminals(stark, p.secret_input):
        p.proof_stream.push(terminal_objects[i])
    p.weights = type(stark)._sample_weights(stark.deep_weight_count(), p.proof_stream.prover_fiat_shamir(), as_array=True)
    if p.secret_input:
        p.weights = secret_input_weights(stark, p.weights)
    S, step = p.shape.S, p.n // p.shape.S
    offset, omega = p.domain.offset.value, p.domain.omega.value
    p.h_values = XArray.empty(S, stark.xfield)
    stark.compose_into(p.h_values, step.bit_length() - 1, p.weights, p.challenges, p.terminals, domain=p.domain)
    p.h_coefficients = XArray.empty(S, stark.xfield)
    raw_ntt(p.h_values.ptr, S, S, p.h_coefficients.ptr, S, S.bit_length() - 1, 3, table_mod._inv(pow(omega, step, P_GOLDILOCKS)), 1, table_mod._inv(S), p.stream)
    _lib.check(_lib.load().bfs_gl_scale(p.h_coefficients.ptr, p.h_coefficients.ptr, S, S, 3, table_mod._inv(offset), p.stream))
    if debug_checks.enabled():
        _check_degree(stark, p)


def _check_degree(stark, p):
    """DEBUG: an honest trace's H has degree < S (every quotient's degree bound is at most max_degree), so H on m >= 2 S points
    interpolates to S coefficients.  The points are all w of the working domain where it has as many; else the kept interpolants are
    extended to a domain of 2 S points, on which the tables' codewords lie for the length of this check."""
    S, f, xf = p.shape.S, stark.field, stark.xfield
    saved = [(t.base_codewords, t.ext_codewords, t._n) for t in stark.tables]
    try:
        domain = p.domain
        if p.n < 2 * S:
            m = 2 * S
            domain = Fri.Domain(f.generator(), f.primitive_nth_root(m), m)
            widths = [(t.base_width, 3 * (t.full_width - t.base_width)) for t in stark.tables]
            buffers = []
            for k, (coefficients, stride) in enumerate(((p.base_coefficients, p.base_stride), (p.ext_coefficients, p.ext_stride))):
                rows = sum(pair[k] for pair in widths)
                buffers.append(DeviceBuffer(rows * m))
                raw_ntt(coefficients.ptr, stride, stride, buffers[k].ptr, m, m.bit_length() - 1, rows, domain.omega.value, domain.offset.value, 1, p.stream)
            at = [0, 0]
            for t, (bw, xw) in zip(stark.tables, widths):
                t.base_codewords, t.ext_codewords, t._n = DeviceView(buffers[0], at[0] * m, bw * m), DeviceView(buffers[1], at[1] * m, xw * m), m
                at = [at[0] + bw, at[1] + xw]
        m = domain.length
        values, coefficients = XArray.empty(m, xf), XArray.empty(m, xf)
        stark.compose_into(values, 0, p.weights, p.challenges, p.terminals, domain=domain)
        raw_ntt(values.ptr, m, m, coefficients.ptr, m, m.bit_length() - 1, 3, table_mod._inv(domain.omega.value), 1, table_mod._inv(m), p.stream)
        assert not coefficients.to_numpy()[:, S:].any(), "the composition polynomial has degree >= S = %d" % S
    finally:
        for t, (base, ext, n) in zip(stark.tables, saved):
            t.base_codewords, t.ext_codewords, t._n = base, ext, n


def _stage_composition_commit(stark, p):
    """C2: the s segments of H -- without segment blinding (m = 0) views of its coefficients, segment i the coefficients [i L, (i + 1) L)
    of each limb plane; with it the pieces of L0 = L - m coefficients blinded by bfsz_split_blind, H_j' = H_j + X^L0 b_j - b_{j-1} with
    uniform b_0 .. b_{s-2} of m coefficients (one draw) -- and, where the shape has one, the masking polynomial R of L uniform
    coefficients (the next draw) as the commitment's last column"""
    from . import debug_checks
    shape, h = p.shape, p.h_coefficients
    L, S, s, m = shape.L, shape.S, shape.s, shape.m
    p.segment_blinding = p.blinded_segments = p.masking_polynomial = None
    if m:
        p.segment_blinding = table_mod.draw_field_words(p.draw, 3 * (s - 1) * m, p.stream)
        p.blinded_segments = DeviceBuffer(3 * s * L)
        _lib.check(_lib.load().bfsz_split_blind(h.ptr, h.stride, S, shape.L0, s, p.segment_blinding.ptr, m, m, p.blinded_segments.ptr, L, p.stream))
        p.segments = [XArray(DeviceView(p.blinded_segments, 3 * i * L, 3 * L), L, stark.xfield, stride=L) for i in range(s)]
    else:
        p.segments = [XArray(DeviceView(h.buf, i * L, 2 * S + L), L, stark.xfield, stride=S) for i in range(s)]
        if debug_checks.enabled():
            assert len(p.segments) * L == len(h) and all(len(f) == L and f.stride == S for f in p.segments), \
                "the segments do not tile the composition polynomial's coefficients"
    committed = list(p.segments)
    if shape.randomizer:
        p.masking_polynomial = XArray(table_mod.draw_field_words(p.draw, 3 * L, p.stream), L, stark.xfield, stride=L)
        committed.append(p.masking_polynomial)
    p.commitments.append(p.pc.commit(committed, p.proof_stream))


def _stage_opening(stark, p):
    """z, drawn behind C2's root, and the one opening of all 25 + s columns"""
    p.z = tuple(stark.xfield.sample(p.proof_stream.prover_fiat_shamir()).limbs())
    if p.z[1] == 0 and p.z[2] == 0:
        raise ValueError("the drawn point lies in the base field (chance 2^-128): prove again")
    p.plan = deep_opening_plan(stark.tables, p.z, segments=p.shape.s, randomizer=p.shape.randomizer)
    p.opened = p.pc.open_rounds(p.commitments, p.plan.groups, p.proof_stream)
    stark._last = {"challenges": p.challenges, "terminals": p.terminals}
    if stark.keep_intermediates:          # the working codewords (w words each) and the committed ones (n words each; the same buffers where w = n)
        stark._last.update({"commitments": p.commitments, "weights": p.weights, "z": p.z, "plan": p.plan, "h_values": p.h_values,
                            "h_coefficients": p.h_coefficients, "base_polys": p.base_polys, "ext_polys": p.ext_polys,
                            "opened": [[[tuple(v.limbs()) for v in per_point] for per_point in per_group] for per_group in p.opened],
                            "segments": p.segments, "L": p.shape.L, "S": p.shape.S, "s": p.shape.s, "working_base_codewords": p.base_codewords,
                            "working_ext_codewords": p.ext_codewords, "committed_base_codewords": p.base_committed,
                            "committed_ext_codewords": p.ext_committed,
                            # the zero-knowledge mode's draws (empty / None without): per table with rows its blinding words, w rows of k
                            "k": p.shape.k, "m": p.shape.m, "L0": p.shape.L0, "base_blinding": p.base_blinding, "ext_blinding": p.ext_blinding,
                            "b": p.segment_blinding, "R": p.masking_polynomial, "blinded_segments": p.blinded_segments})
    else:
        type(stark)._release(*stark.tables)


# ---- the verifier
def verify(stark, proof, shape, secret_input=False):
    """BrainfuckStark.verify_deep on `shape`: False with one printed line for every refusal, a malformed stream included; raises nothing
    (but the ValueErrors of check_secret_input, which are about the call and not about the proof)"""
    if secret_input:
        check_secret_input(stark, shape)
    try:
        return _verify_stream(stark, ProofStream().deserialize(proof), shape, secret_input)
    except Exception as e:          # whatever a stream that is not prove_deep's makes the readers raise
        print("malformed proof: %s" % type(e).__name__)
        return False


def _verify_stream(stark, proof_stream, shape, secret_input=False):
    X0, X1, xadd, xsub, xmul, xinv, xpow = air.X0, air.X1, air.xadd, air.xsub, air.xmul, air.xinv, air.xpow
    canonical_limbs, sample_weights = type(stark)._canonical_limbs, type(stark)._sample_weights
    root0 = proof_stream.pull()
    challenges = tuple(sample_weights(11, proof_stream.verifier_fiat_shamir()))
    root1 = proof_stream.pull()
    # the terminals the stream carries; the slot of one it does not carry (the secret input's evaluation) holds zero and is compared with nothing
    sent = sent_terminals(stark, secret_input)
    terminals, stored = [X0] * 5, [X0] * 5
    for i in sent:
        t = proof_stream.pull()
        terminals[i] = canonical_limbs(t)
        stored[i] = tuple(t.limbs()) if hasattr(t, "limbs") else (t.value, 0, 0)
    checked = [(io, ea) for io, ea in zip((stark.input_table, stark.output_table, None), stark.evaluation_arguments) if ea.terminal_index in sent]
    for io, ea in checked:          # the rule of _verify_head, as a refusal
        if io is not None and io.height != 0 and not any(stored[io.terminal_index]) and any(ea.compute_terminal(challenges)):
            print("evaluation terminal of a non-empty input or output table is zero")
            return False
    for _, ea in checked:
        if tuple(ea.select_terminal(stored)) != tuple(ea.compute_terminal(challenges)):
            print("a terminal does not match the public input, output or program")
            return False
    weights = sample_weights(stark.deep_weight_count(), proof_stream.verifier_fiat_shamir())
    if secret_input:
        weights = secret_input_weights(stark, weights)
    root2 = proof_stream.pull()
    if not isinstance(root2, (bytes, bytearray)):          # (a proof with another number of terminals: a terminal lies where this mode's root does)
        print("the composition's root is not a digest")
        return False
    z = tuple(stark.xfield.sample(proof_stream.verifier_fiat_shamir()).limbs())
    if z[1] == 0 and z[2] == 0:
        print("the drawn point lies in the base field")
        return False
    plan = deep_opening_plan(stark.tables, z, segments=shape.s, randomizer=shape.randomizer)
    values = PolynomialCommitment(shape.fri, hiding=shape.hiding).read_rounds([root0, root1, root2], plan.widths, plan.groups, proof_stream)
    if values is None:
        return False
    if plan.empty_group is not None and any(any(v) for v in values[plan.empty_group][0]):
        print("a column of a table without rows is not zero")
        return False
    total, at, rows = X0, 0, []
    boundary = xinv(xsub(z, X1))
    for t, g in zip(stark.tables, plan.table_group):
        if g is None:
            rows.append([X0] * t.full_width)
            at += t.num_quotients()
            continue
        cur = values[g][0]
        nxt = values[g][1] if len(values[g]) > 1 else cur          # height 1: the next row is the row itself
        rows.append(cur)
        off = xsub(z, (table_mod._inv(t.omicron.value), 0, 0))
        factors = {"boundary": boundary, "transition": xmul(off, xinv(xsub(xpow(z, t.height), X1))), "terminal": xinv(off)}
        params, memo = t.air_params(challenges), {}
        for kind, constraints in t.air.all():
            for e in constraints:
                value = air.evaluate(e, cur, nxt, challenges, terminals, params, memo)
                total = xadd(total, xmul(xmul(weights[at], value), factors[kind]))
                at += 1
    for j, pa in enumerate(stark.permutation_arguments):
        total = xadd(total, xmul(xmul(weights[at + j], pa.evaluate_difference(rows)), boundary))
    h_at_z, z_to_L = X0, xpow(z, shape.L0)
    for segment in reversed(values[plan.h_group][0][:shape.s]):          # Horner in z^L0 over the segments' values (a masking polynomial's value behind them is the opening's alone)
        h_at_z = xadd(xmul(h_at_z, z_to_L), tuple(segment))
    if total != h_at_z:
        print("the composition polynomial does not match the opened rows")
        return False
    return True
