"""STARK prover for the Brainfuck VM -- mirror of the reference's `brainfuck_stark.py`
(/root/reference/code/brainfuck_stark.py:20-341): same constructor, `prove(...)`, `get_terminals`, `sample_weights`,
`sample_indices`, and the same transcript, byte for byte.

Where the time goes in the reference, and where it goes here:
  trace interpolation + low-degree extension (:165-172, 194-195)    batched INTT / randomizer fix / coset NTT in HBM (table.py)
  table extension: running products / evaluations (:186-187)        prefix scans on the trace columns in HBM (bfs_xfe_scan_device)
  commitments to zipped codewords (:178-179, 197-198)               row pickles synthesised and hashed on the GPU (bfs_merkle_build_rows)
  quotient codewords (:204-221, 93 % of the reference's time)       one kernel per table, folded straight into ...
  non-linear combination of 151 terms (:236-298)                    ... the combination accumulator (bfs_air_combine); with
                                                                    keep_intermediates the quotients are written out (bfs_air_quotients,
                                                                    bfs_combination) so that tests can compare each with the reference's
  FRI (:336)                                                        fri.Fri.prove (bfs_fri_commit / bfs_fri_query), round 0 on the
                                                                    combination tree that was just built
Padding, Fiat-Shamir sampling, transcript assembly and the object-identity bookkeeping of opened rows stay on the host.

The second protocol, proving by out-of-domain openings (prove_deep / verify_deep and their two domain shapes), which the reference has
no counterpart for, lives in deep_stark.py; the methods of that name here hand over to it, and it reaches back through the object.
"""
import ctypes
import gc
import os
import time
from hashlib import blake2b
from types import SimpleNamespace

import numpy as np
from os import urandom          # module-level on purpose: tests patch `brainfuck_stark.urandom` for determinism
from .randomness import source as random_source

from . import _lib, air, arrays, deep_stark, salted_merkle as salted_mod, table as table_mod
from .algebra import BaseField, BaseFieldElement
from .arrays import XArray
from .deep_stark import deep_opening_plan          # (importable from here as before)
from .device import GatherBatch, current_stream, gather, synchronize
from .evaluation_argument import EvaluationArgument, ProgramEvaluationArgument
from .extension_field import ExtensionField, ExtensionFieldElement
from .fri import MAX_GRINDING_BITS, Fri
from .instruction_table import InstructionTable
from .io_table import InputTable, OutputTable
from .ip import ProofStream
from .memory_table import MemoryTable
from .merkle import CosetMerkle, Merkle, leaf_pickle_source
from .permutation_argument import PermutationArgument
from .processor_table import ProcessorTable
from .salted_merkle import SaltedMerkle, ZippedSaltedMerkle
from .algebra import P_GOLDILOCKS
from .table import (AirViolation, AirViolationError, extend_tables_device, lde_tables, prepare_extension, sample_ext, sample_ext_many,
                    zerofier_inverses)
from .univariate import Polynomial
from .vm import VirtualMachine

_u64 = ctypes.c_uint64


class _MalformedProof(Exception):
    """an object in the proof is not what its position requires (verify() answers False)"""


def _canonical_limbs(e):
    """value of an element read from the proof, as canonical residues: the prover chooses the representation (any Python int
    unpickles), the reference reduces in every operation (algebra.py:89-99) and so sees v mod p -- and so must every
    consumer here: bfs_air_evaluate's host arithmetic assumes canonical operands and ctypes truncates above 2^64.  An extension
    element with more than three coefficients is not an element: the proof is refused."""
    if hasattr(e, "limbs"):
        c = e.limbs()
        if len(c) != 3:
            raise _MalformedProof("extension element with %d coefficients" % len(c))
        return (c[0] % air.P, c[1] % air.P, c[2] % air.P)
    return (e.value % air.P, 0, 0)


def _triples(raw, count):
    """`count` extension elements out of a flat array of u64 limbs, as int triples"""
    return [(raw[3 * i], raw[3 * i + 1], raw[3 * i + 2]) for i in range(count)]


def _seed_or_stream(draw, nbytes):
    """a block of random bytes as (seed, None) in production -- 32 bytes of the system's (or the ranks' shared) randomness, which the
    device expands -- or as (None, bytes) when a test replaced urandom: the `nbytes` the reference draws, from the reference's byte stream"""
    if draw is os.urandom or getattr(draw, "expand_on_device", False):
        return draw(32), None
    return None, draw(nbytes)


class _TermLayout:
    """The order of the terms of the non-linear combination (:245-293), which is also the order of the columns in the zipped rows:
    tables in the order of `tables`, all base columns, then all extension columns, then every table's quotients (boundary /
    transition / terminal), then one quotient per permutation argument.  Term s has the weights 1 + 2s and 2 + 2s (weight 0 is the
    randomizer codeword's); column s is element 1 + s of an opened row (element 0 is the randomizer codeword's)."""

    def __init__(self, tables, permutation_arguments, max_degree):
        self.tables, self.max_degree = tables, max_degree
        self.num_base = sum(self.width(t, 0) for t in tables)
        self.num_columns = self.num_base + sum(self.width(t, 1) for t in tables)
        self.base, self.ext, self.quot = [], [], []          # per table: its slice of the terms
        base_at, ext_at, quot_at = 0, self.num_base, self.num_columns
        for t in tables:
            bw, xw, nq = self.width(t, 0), self.width(t, 1), t.num_quotients()
            self.base.append(slice(base_at, base_at + bw))
            self.ext.append(slice(ext_at, ext_at + xw))
            self.quot.append(slice(quot_at, quot_at + nq))
            base_at, ext_at, quot_at = base_at + bw, ext_at + xw, quot_at + nq
        self.first_argument = quot_at                        # the term of permutation argument j is first_argument + j
        self.weight_count = 1 + 2 * (quot_at + len(permutation_arguments))          # the randomizer codeword's, then two per term

    @staticmethod
    def width(table, ext):
        return table.full_width - table.base_width if ext else table.base_width

    def column_degree_bounds(self):
        """the interpolant's degree bound per base column, then per extension column (heights are final once the tables are padded)"""
        return [t.interpolant_degree() for ext in (0, 1) for t in self.tables for _ in range(self.width(t, ext))]

    def shifts(self, quotient_bounds):
        """per term, the power of x that lifts it to the common degree bound: the columns, then the quotients"""
        return [self.max_degree - b for b in self.column_degree_bounds() + list(quotient_bounds)]

    def unit_distances(self, n):
        """the distances from an opened index to the rows opened with it.  The iteration order of this very expression is part of the
        proof format: the rows are pushed in it, and native prover and verifier are handed the list as it comes out."""
        return list(set(table.unit_distance(n) for table in self.tables))

    def device_columns(self, n, ext):
        """every base (ext = 0) or extension (ext = 1) column codeword in HBM, in term order: (table, column, address, limbs).  A
        table's columns lie `limbs * n` words apart."""
        out = []
        for t in self.tables:
            buf, limbs = (t.ext_codewords, 3) if ext else (t.base_codewords, 1)
            out += [(t, c, buf.ptr + 8 * limbs * c * n, limbs) for c in range(self.width(t, ext))]
        return out

    def row_requests(self, n, ext, i):
        """gather requests (address, words, stride) for row i of those columns: one per table, from its first column on"""
        return [(address + 8 * i, limbs * self.width(t, ext), n) for t, c, address, limbs in self.device_columns(n, ext) if c == 0]


class _RowBuilder:
    """Opened rows of the two zipped trees as the objects the reference pickles (only opened rows are ever read back).  The trees keep
    its methods in their lazy leaf lists, so it outlives prove(): it must not hold the prover, or a prover object kept with its trees
    (keep_intermediates) becomes a reference cycle and its HBM waits for a full garbage collection."""

    def __init__(self, layout, n, randomizer_codeword, field, xfield):
        self.layout, self.n, self.randomizer_codeword, self.field, self.xfield = layout, n, randomizer_codeword, field, xfield
        self.fetched_base, self.fetched_ext = {}, {}      # row -> words, filled by the batched gather of the openings
        self.fastlist = arrays._fastlist                  # the same objects, made in C (cpyext/fastlist.c): 16 elements in 3 us instead of 16
        self.internal = xfield.modulus.coefficients[0].field
        self.moduli = self.shared = self.plain_columns = None

    def share(self, moduli):
        """moduli: per extension column, None or the period with which its elements share coefficient objects (Table.ext_sharing_moduli)"""
        self.moduli = moduli
        self.shared = [dict() for _ in moduli]            # per column: i mod modulus -> the coefficient objects of that class
        self.plain_columns = [c for c in range(len(moduli)) if moduli[c] is None]

    def requests(self, ext, i):
        """gather requests for row i of the base tree (ext = 0: the randomizer codeword, then the base columns) or the extension tree"""
        rc = self.randomizer_codeword
        return ([] if ext else [(rc.ptr + 8 * i, 3, rc.stride)]) + self.layout.row_requests(self.n, ext, i)

    def base_row(self, i):
        words = self.fetched_base[i] if i in self.fetched_base else gather(self.requests(0, i))
        if self.fastlist is not None:
            tail = self.fastlist.unpack_base(np.ascontiguousarray(words[3:], dtype=np.uint64), BaseFieldElement, self.field)
        else:
            tail = [BaseFieldElement(int(v), self.field) for v in words[3:]]
        return tuple([self.xfield.from_limbs([int(v) for v in words[:3]])] + tail)

    def ext_row(self, i):
        xf, moduli, columns = self.xfield, self.moduli, self.layout.num_columns - self.layout.num_base
        words = self.fetched_ext[i] if i in self.fetched_ext else gather(self.requests(1, i))
        row, made = [], {}          # made: column -> element, for those made in C
        if self.fastlist is not None and self.plain_columns:
            # the elements without shared coefficient objects, all at once: limb planes (3, k) -> k ExtensionFieldElements
            soa = np.ascontiguousarray(np.asarray(words, dtype=np.uint64).reshape(columns, 3)[self.plain_columns].T)
            made = dict(zip(self.plain_columns, self.fastlist.unpack_ext(soa, ExtensionFieldElement, Polynomial, BaseFieldElement, xf, self.internal)))
        for c in range(columns):
            limbs = [int(v) for v in words[3 * c:3 * c + 3]]
            if c in made:
                row.append(made[c])
            elif moduli[c] is None:
                row.append(xf.from_limbs(limbs))
            else:
                while limbs and limbs[-1] == 0:
                    limbs.pop()
                objs = self.shared[c].setdefault(i % moduli[c], [BaseFieldElement(v, self.internal) for v in limbs])
                e = ExtensionFieldElement(Polynomial(objs), xf)
                e.shares_coefficients = True
                row.append(e)
        return tuple(row)


class BrainfuckStark:
    field = BaseField.main()
    xfield = ExtensionField.main()

    def __init__(self, running_time, memory_length, program, input_symbols, output_symbols, log_expansion_factor=2, security_level=2,
                 folding_factor=2, coset_leaves=False, grinding_bits=0):
        """the reference fixes log_expansion_factor = 2 and security_level = 2 "for speed" (brainfuck_stark.py:31-36, with 4 and 160
        commented as the real values); they are parameters here, the defaults reproduce the reference.

        folding_factor (2, 4 or 8), coset_leaves and grinding_bits (0..40) go to `Fri` unchanged (fri.py explains them; its assertions
        fire here) and decide how the combination codeword is committed to and tested; the defaults are the reference's protocol,
        byte for byte.  With coset_leaves the commitment to the combination codeword is CosetMerkle(combination, folding_factor) and
        every opened index reveals the coset tuple it lies in with one path ("FRI modes at the STARK level").
        grinding_bits = b buys b bits of FRI's conjectured security with a proof of work, so FRI runs
        (security_level - b) // log_expansion_factor colinearity checks.  The number of row indices the STARK itself opens stays
        security_level: grinding protects only FRI's query sampling, the only sampling that follows the nonce -- the row indices are
        drawn before FRI begins, so a prover re-rolls them without paying for a nonce."""
        self.running_time = running_time
        self.memory_length = memory_length
        self.program = program
        self.input_symbols = input_symbols
        self.output_symbols = output_symbols

        self.expansion_factor = 1 << log_expansion_factor
        self.security_level = security_level
        assert type(grinding_bits) is int and 0 <= grinding_bits <= MAX_GRINDING_BITS, "grinding_bits must be an int from 0 to 40"
        self.num_colinearity_checks = (self.security_level - grinding_bits) // log_expansion_factor
        assert self.expansion_factor & (self.expansion_factor - 1) == 0, "expansion factor must be a power of 2"
        assert self.expansion_factor >= 4, "expansion factor must be 4 or greater"
        if grinding_bits == 0:
            assert self.num_colinearity_checks * log_expansion_factor >= self.security_level, \
                "number of colinearity checks times log of expansion factor must be at least security level"
        else:
            assert self.num_colinearity_checks * log_expansion_factor + grinding_bits >= self.security_level, \
                "number of colinearity checks times log of expansion factor plus grinding bits must be at least security level"
            assert self.num_colinearity_checks >= 1, "grinding bits must leave at least one colinearity check"
        self.num_randomizers = 1

        order = 1 << 32
        smooth_generator = BrainfuckStark.field.primitive_nth_root(order)
        f = self.field
        self.processor_table = ProcessorTable(f, running_time, self.num_randomizers, smooth_generator, order)
        self.instruction_table = InstructionTable(f, running_time + len(program), self.num_randomizers, smooth_generator, order)
        self.memory_table = MemoryTable(f, memory_length, self.num_randomizers, smooth_generator, order)
        self.input_table = InputTable(f, len(input_symbols), smooth_generator, order)
        self.output_table = OutputTable(f, len(output_symbols), smooth_generator, order)
        self.tables = [self.processor_table, self.instruction_table, self.memory_table, self.input_table, self.output_table]

        self.permutation_arguments = [
            PermutationArgument(self.tables, (0, ProcessorTable.instruction_permutation), (1, InstructionTable.permutation)),
            PermutationArgument(self.tables, (0, ProcessorTable.memory_permutation), (2, MemoryTable.permutation))]
        self.evaluation_arguments = [
            EvaluationArgument(8, 2, [BaseFieldElement(ord(i), f) for i in input_symbols]),
            EvaluationArgument(9, 3, [BaseFieldElement(ord(o), f) for o in output_symbols]),
            ProgramEvaluationArgument([0, 1, 2, 10], 4, program)]

        # FRI domain length from the degree of the composed transition constraints (:82-95)
        self.max_degree = 1
        ones = [air.X1] * 11
        for table in self.tables:
            self.max_degree = max(self.max_degree, table.max_transition_degree(ones))
        self.max_degree = BrainfuckStark.roundup_npo2(self.max_degree) - 1
        fri_domain_length = (self.max_degree + 1) * self.expansion_factor
        generator = BrainfuckStark.field.generator()
        omega = BrainfuckStark.field.primitive_nth_root(fri_domain_length)
        self.fri = Fri(generator, omega, fri_domain_length, self.expansion_factor, self.num_colinearity_checks, self.xfield,
                       folding_factor=folding_factor, coset_leaves=coset_leaves, grinding_bits=grinding_bits)
        self._default_fri = folding_factor == 2 and not coset_leaves and grinding_bits == 0          # the reference's protocol
        self._layout = _TermLayout(self.tables, self.permutation_arguments, self.max_degree)
        self._segmented_fri = {}          # domain length -> the second Fri of the segmented prove_deep / verify_deep (deep_segmented_shape)

    def get_terminals(self):
        """the five terminals as int triples (:103-109)"""
        return [self.processor_table.instruction_permutation_terminal, self.processor_table.memory_permutation_terminal,
                self.processor_table.input_evaluation_terminal, self.processor_table.output_evaluation_terminal,
                self.instruction_table.evaluation_terminal]

    @staticmethod
    def _sample_weights(number, randomness, as_array=False):
        """:104-112: weight i = ExtensionField.sample(blake2b(randomness + bytes(i)).digest()), i.e. the three 21-byte big-endian
        chunks of the digest mod p (extension_field.py:100-111; the 64th byte is not used).  One integer conversion per digest."""
        if number > 4:             # natively (bfs_sample_weights): 157 digests and 471 reductions are ~150 us of a 4 ms proof in Python
            lib = _lib.load()
            raw = (ctypes.c_uint64 * (3 * number))()
            randomness = bytes(randomness)
            _lib.check(lib.bfs_sample_weights(randomness, len(randomness), number, raw))
            if as_array:           # (number, 3) uint64: the prover hands the weights on to the kernels as they are
                return np.frombuffer(raw, dtype=np.uint64).reshape(number, 3)
            flat = list(raw)
            return [(flat[3 * i], flat[3 * i + 1], flat[3 * i + 2]) for i in range(number)]
        out, mask = [], (1 << 168) - 1
        for i in range(number):
            v = int.from_bytes(blake2b(randomness + bytes(i)).digest()[:63], "big")
            out.append(((v >> 336) % P_GOLDILOCKS, ((v >> 168) & mask) % P_GOLDILOCKS, (v & mask) % P_GOLDILOCKS))
        return np.array(out, dtype=np.uint64).reshape(number, 3) if as_array else out

    def sample_weights(self, number, randomness):
        """:111-112, as extension-field element objects"""
        return [self.xfield.from_limbs(w) for w in BrainfuckStark._sample_weights(number, randomness)]

    @staticmethod
    def sample_indices(number, randomness, bound):
        """:114-123"""
        return [int.from_bytes(blake2b(randomness + bytes(i)).digest(), "big") % bound for i in range(number)]

    @staticmethod
    def roundup_npo2(integer):
        if integer == 0 or integer == 1:
            return 1
        return 1 << (integer - 1).bit_length()

    # ------------------------------------------------------------------------------------------------------------
    keep_intermediates = False      # True: prove() leaves trees, quotient codewords and the combination codeword in `_last` (tests)
    stage_timing = False            # True: prove() synchronises its stream after every stage so that `timing` splits the GPU time by stage
                                    # (bench.py's breakdown, tools/); False: `timing` holds host time per stage and the stages overlap freely
    check_air = False               # True: prove() takes the Python stage path and checks the full AIR on the extended trace in HBM
                                    # (bfs_air_check) before any quotient or FRI work; a violation raises AirViolationError

    # ---- several GPUs on one proof (shard.RowShardedSaltedMerkle): every rank runs the polynomial stages on all columns and hashes
    # only its range of the zipped rows; set by cooperate() and used inside shard.shared_randomness()
    _cooperation = None
    _row_windows = None      # tests: [(first, count), ...] tiling the FRI domain, in any order -- the combination stage runs window by window
    _shift_tweak = None      # tests: shifts -> shifts, applied to the combination's degree shifts (both combination paths see the result)

    def cooperate(self, world_size, rank, group=None, device=None):
        """this prover is one of `world_size` identical provers (one per GPU) working on the SAME proof: the zipped commitments are
        built cooperatively, every rank returns the same proof bytes.  Call prove() inside `with shard.shared_randomness(...)`."""
        assert self._default_fri, "cooperate() proves with the default FRI mode only (folding_factor=2, coset_leaves=False, grinding_bits=0)"
        self._cooperation = (int(world_size), int(rank), group, device) if world_size > 1 else None
        return self

    def _zipped_tree(self, columns, n, make_row):
        if self._cooperation is None:
            return ZippedSaltedMerkle(columns, n, make_row)
        from .shard import RowShardedSaltedMerkle
        world_size, rank, group, device = self._cooperation
        return RowShardedSaltedMerkle(columns, n, make_row, world_size, rank, group=group, device=device)

    def _openings_python(self, p):
        """the openings (:315-333) through Python objects: used when the transcript cannot take them natively (a foreign proof
        stream class, the row-sharded trees of a cooperative proof)"""
        proof_stream, base_tree, extension_tree, combination_tree, n = p.proof_stream, p.base_tree, p.extension_tree, p.combination_tree, p.n
        distances = [0] + p.unit_distances
        # everything the openings read from HBM -- rows, salts, authentication paths, combination leaves -- in one round trip
        rows = list(dict.fromkeys((index + distance) % n for index in p.indices for distance in distances))
        batch = GatherBatch()
        row_tickets = {i: ([batch.add(*r) for r in p.rows.requests(0, i)], [batch.add(*r) for r in p.rows.requests(1, i)]) for i in rows}
        # (coset leaves: per opened coset c = index mod q its a elements c + j q, and the path of leaf c)
        coset = self.fri.coset_leaves
        a, q = (self.fri.folding_factor, n // self.fri.folding_factor) if coset else (1, n)
        leaf_tickets = {c: [batch.add(p.combination.ptr + 8 * (c + j * q), 3, p.combination.stride) for j in range(a)]
                        for c in dict.fromkeys(index % q for index in p.indices)}
        stores = [base_tree.prefetch_salts(rows, batch), extension_tree.prefetch_salts(rows, batch),
                  base_tree.prefetch_paths(rows, batch), extension_tree.prefetch_paths(rows, batch),
                  combination_tree.prefetch_paths([index % q for index in p.indices], batch)]
        batch.run()
        for store in stores:
            store()
        for i, (tb, te) in row_tickets.items():
            p.rows.fetched_base[i] = np.concatenate([batch.words(t) for t in tb])
            p.rows.fetched_ext[i] = np.concatenate([batch.words(t) for t in te])
        for index in p.indices:
            for distance in distances:
                idx = (index + distance) % n
                proof_stream.push(base_tree.leafs[idx][0])
                proof_stream.push(base_tree.open(idx))
                proof_stream.push(extension_tree.leafs[idx][0])
                proof_stream.push(extension_tree.open(idx))
        known = {}
        for index in p.indices:
            c = index % q
            if c not in known:                       # the same index twice is the same leaf object twice -- and so is a coset two indices share
                elements = [self.xfield.from_limbs([int(v) for v in batch.words(ticket)]) for ticket in leaf_tickets[c]]
                known[c] = tuple(elements) if coset else elements[0]
            proof_stream.push(known[c])
            proof_stream.push(combination_tree.open(c))
        return {} if coset else known                # (a Fri that commits to cosets opens whole cosets itself: nothing to alias)

    def _openings_native(self, p):
        """the same through bfs_stark_push_openings: rows, salts, paths and leaves go from HBM into the native transcript in one
        call, and become Python objects only if somebody looks at proof_stream.objects (ip.ProofStream._adopt_lazy).  Returns
        {index: handle of the combination leaf} for Fri.prove, or None when this route is not available."""
        base_tree, extension_tree, combination, combination_tree, xf = p.base_tree, p.extension_tree, p.combination, p.combination_tree, self.xfield
        coset = self.fri.coset_leaves
        if (self._cooperation is not None or type(base_tree) is not ZippedSaltedMerkle or type(extension_tree) is not ZippedSaltedMerkle
                or combination_tree._nodes_host is not None or combination_tree.num_leafs != (p.n // self.fri.folding_factor if coset else p.n)):
            return None
        transcript = BrainfuckStark._native_transcript(p.proof_stream, xf)
        if transcript is None:
            return None

        def requests(reqs):
            arr = (_lib.GatherRequest * len(reqs))()
            for a, (ptr, nwords, stride) in zip(arr, reqs):
                a.d_base, a.nwords, a.stride, a.out_offset = ptr, nwords, stride, 0
            return arr

        def salts(tree):
            if getattr(tree, "_salt_cache", None) is not None:
                return ctypes.c_void_p(tree._salt_base), 1
            return ctypes.c_void_p(ctypes.addressof(tree._salt_host)), 0
        base_arr, ext_arr = requests(p.rows.requests(0, 0)), requests(p.rows.requests(1, 0))
        moduli, indices = p.rows.moduli, p.indices
        mods = (_u64 * max(len(moduli), 1))(*[0 if m is None else int(m) for m in moduli])
        idx = (_u64 * len(indices))(*indices)
        dist = (_u64 * (1 + len(p.unit_distances)))(0, *p.unit_distances)
        out = (_u64 * len(indices))()
        (bs, bs_dev), (es, es_dev) = salts(base_tree), salts(extension_tree)
        before = transcript.num_objects()
        head = (transcript.handle, base_arr, len(base_arr), transcript._field_id(BrainfuckStark.field), ext_arr, len(ext_arr), mods, len(moduli), p.n,
                base_tree._nodes.ptr, bs, bs_dev, extension_tree._nodes.ptr, es, es_dev, combination.ptr, combination.stride,
                combination_tree._nodes.ptr)
        if coset:          # the coset tuples and their paths (bfs_stark_push_openings_cosets); FRI takes no aliases in this form
            _lib.check(_lib.load().bfs_stark_push_openings_cosets(*head, self.fri._log2_folding, idx, len(indices), dist, len(dist), p.stream))
        else:
            _lib.check(_lib.load().bfs_stark_push_openings(*head, idx, len(indices), dist, len(dist), out, p.stream))
        p.proof_stream._adopt_lazy(transcript, before, transcript.num_objects(), xf)
        return {} if coset else {index: int(handle) for index, handle in zip(indices, out)}

    @staticmethod
    def _native_transcript(proof_stream, xf, refuse_loaded=False):
        """the native transcript of `proof_stream` if native code may append objects of extension field `xf` to it (the field is
        claimed on first use), else None: a foreign proof stream, a transcript that is not the stream's cached one or belongs to
        another field -- and, for a caller that has to map Python objects to handles, one that was read natively from bytes"""
        if not hasattr(proof_stream, "_adopt_lazy"):
            return None
        transcript = proof_stream._native()
        if getattr(proof_stream, "_cached", None) is not transcript or (transcript.xfield is not None and transcript.xfield is not xf):
            return None
        if refuse_loaded and transcript.loaded:
            return None
        if transcript.xfield is None:
            transcript.xfield = xf
        return transcript

    @staticmethod
    def _release(*holders):
        """hand device memory back to the pool now instead of when the garbage collector gets to it (the blocks are
        stream-ordered: kernels already queued keep reading them, the next proof on this stream reuses them)"""
        for h in holders:
            for name in ("buf", "_nodes", "_salts", "base_codewords", "ext_codewords", "_base_device", "_ext_device"):
                b = getattr(h, name, None)
                if hasattr(b, "free"):
                    b.free()
                    if name.endswith("codewords") or name.endswith("_device"):
                        setattr(h, name, None)
            if hasattr(h, "free"):
                h.free()

    def prove(self, program, processor_matrix, memory_matrix, instruction_matrix, input_matrix, output_matrix, proof_stream=None):
        # The trace matrices keep ~10^5 element objects alive; every full garbage collection during (or right after) the proof
        # would walk all of them (measured: 20 ms pauses on a 17 ms proof).  gc.freeze() parks everything that exists now in a
        # permanent generation for the duration of the call; objects made by the proof itself are collected as usual.
        from . import debug_checks
        # DEBUG (the reference's switch, brainfuck_stark.py:251-290, table.py:170-176 / 219-234 / 264-284) or BFS_DEBUG=1: every
        # quotient and every term of the combination is interpolated and its degree asserted (debug_checks.py).  The checks need the
        # quotient codewords in HBM, i.e. the path that keeps intermediates; the proof bytes are the same.
        debug = debug_checks.enabled() and not self.keep_intermediates
        if debug:
            self.keep_intermediates = True
        gc.freeze()
        try:
            return self._prove(program, processor_matrix, memory_matrix, instruction_matrix, input_matrix, output_matrix, proof_stream)
        finally:
            gc.unfreeze()
            if debug:
                self.keep_intermediates = False
                self._last = {k: v for k, v in getattr(self, "_last", {}).items()
                              if k in ("challenges", "terminals", "indices", "weights_seed", "quotient_degree_bounds")}

    # ---- the production path: the stages between the Fiat-Shamir points run natively (csrc/prover.cpp), two calls per proof
    native_stages = True            # False: every stage is driven from Python (the path below; what the tests compare the native one with)

    # one native session per proving THREAD (made on a thread's first proof, freed with the thread).  The threading.local itself is made
    # HERE, once, when the class is defined: made lazily, two threads entering their first prove() together could each create one, and the
    # loser's holder -- referenced from nothing but its own frame -- was finalised (bfs_stark_session_free) while the thread still proved
    # with the freed session (round-5 advice).
    _thread_sessions = __import__("threading").local()

    @staticmethod
    def _native_session():
        """the calling thread's bfs_stark session.  A session owns side streams, events and scratch buffers (csrc/prover.cpp), which
        cost far more to make than a small proof takes, so it belongs to the thread, not to the BrainfuckStark object: provers are
        made per claim (running time, program, symbols) and thrown away, threads stay."""
        import weakref
        local = BrainfuckStark._thread_sessions
        holder = getattr(local, "holder", None)
        if holder is None:
            lib = _lib.load()

            class _Holder:
                pass
            holder = local.holder = _Holder()
            holder.session = lib.bfs_stark_session_new()
            weakref.finalize(holder, lib.bfs_stark_session_free, holder.session)
        return holder.session

    @staticmethod
    def _matrix_values(matrix, width):
        """the uint64 array behind a trace matrix of this package's VM (rows x >= width, C order), or None for plain lists of rows"""
        values = getattr(matrix, "values", None)
        if values is None or not isinstance(values, np.ndarray) or values.dtype != np.uint64 or values.ndim != 2:
            return None
        if values.shape[0] != len(matrix) or (values.shape[0] and (values.shape[1] < width or not values.flags.c_contiguous)):
            return None
        return values

    def _native_randomness(self, n):
        """every random draw of prove(), in its order, from the sources the Python path reads (tests replace them module by module), as
        the structure bfs_stark_commit takes.  Returns (structure, buffers it points at): keep the second alive as long as the first."""
        rnd = _lib.StarkRandomness()
        keep = []                                                               # buffers the structure points at (ADDRESSES go into it:
        # ctypes.cast(buffer, c_void_p) puts the buffer into its own _objects dictionary -- a reference cycle, and a 24 n-byte salt
        # buffer per commitment then lives until the cyclic collector happens to run: a soak grew by 5 MB per proof that way)
        draw = random_source(urandom)
        count = self.max_degree + 1
        seed, blob = _seed_or_stream(draw, 3 * 9 * count)        # the randomizer polynomial (:162-165): `count` draws of 27 bytes
        if seed is not None:
            keep.append(ctypes.create_string_buffer(seed, 32))
            rnd.randomizer_seed = ctypes.addressof(keep[-1])
        else:
            keep.append(np.ascontiguousarray(sample_ext_many(blob, count, 9), dtype=np.uint64))
            rnd.randomizer_limbs = keep[-1].ctypes.data
        tdraw = random_source(table_mod.urandom)

        def draws(source, count):
            """`count` draws of 24 bytes (table.py:125-127), as integers; the operating system's generator is asked once for all of them"""
            if source is os.urandom:
                blob = source(24 * count)
                return [int.from_bytes(blob[24 * i:24 * i + 24], "big") for i in range(count)]
            return [int.from_bytes(source(24), "big") for _ in range(count)]
        base_rand = [v % P_GOLDILOCKS for v in draws(tdraw, sum(t.base_width for t in self.tables[:3] if t.height))]
        keep.append((_u64 * max(len(base_rand), 1))(*base_rand))
        rnd.base_randomizers = ctypes.addressof(keep[-1])

        def salts(field_seed, field_data):
            seed, data = _seed_or_stream(random_source(salted_mod.urandom), 24 * n)
            keep.append(ctypes.create_string_buffer(seed or data, len(seed or data)))
            setattr(rnd, field_data if seed is None else field_seed, ctypes.addressof(keep[-1]))
        salts("base_salt_seed", "base_salts")
        initials = [sample_ext(draw(3 * 8)) for _ in self.permutation_arguments]
        rnd.initials = (_u64 * 6)(*[v for i in initials for v in i])
        mask64 = (1 << 64) - 1              # ExtensionField.sample of 24 bytes: three big-endian 8-byte chunks mod p (extension_field.py:100-111)
        ext_rand = [c % P_GOLDILOCKS for v in draws(tdraw, sum(t.full_width - t.base_width for t in self.tables[:3] if t.height))
                    for c in (v >> 128, (v >> 64) & mask64, v & mask64)]
        keep.append((_u64 * max(len(ext_rand), 1))(*ext_rand))
        rnd.ext_randomizers = ctypes.addressof(keep[-1])
        salts("ext_salt_seed", "ext_salts")
        return rnd, keep

    def _adopt_commit_reply(self, out_ch, out_scan, out_io, ci):
        """what bfs_stark_commit answered -- 11 challenges, the 7 terminals of its scans with 2 spare, the 2 IO tables' -- onto the
        tables, as the Python path's extension leaves them (ci: the processor's current-instruction column); returns (challenges,
        terminals, terminal objects)"""
        challenges = tuple(_triples(out_ch, 11))
        scan, io = _triples(out_scan, 9), _triples(out_io, 2)
        pt, it, mt = self.processor_table, self.instruction_table, self.memory_table
        (pt.instruction_permutation_terminal, pt.memory_permutation_terminal, pt.input_evaluation_terminal,
         pt.output_evaluation_terminal) = scan[0:4]
        it.permutation_terminal, it.evaluation_terminal = scan[4], scan[5]
        mt.permutation_terminal = scan[6]
        self.input_table.evaluation_terminal, self.output_table.evaluation_terminal = io
        pt.evaluation_terminal_identities = (pt._identity(None, scan[2], challenges[8], np.nonzero(ci == ord(","))[0] + 1),
                                             pt._identity(None, scan[3], challenges[9], np.nonzero(ci == ord("."))[0]))
        terminals = self.get_terminals()
        return challenges, terminals, self._terminal_objects(terminals)

    def _prove_native(self, program, matrices, proof_stream):
        """prove() through bfs_stark_commit / bfs_stark_finish.  Returns the proof bytes, or None when this route does not apply (the
        caller then takes the Python path): plain-list matrices, a foreign proof stream, a cooperative proof, test hooks."""
        if os.environ.get("BFS_NATIVE_PROVE", "1") == "0" or not self.native_stages:
            return None
        if (self._cooperation is not None or self.keep_intermediates or self.stage_timing or self.check_air or self._row_windows is not None
                or self._shift_tweak is not None):
            return None
        # tables in the order of self.tables: processor, instruction, memory, input, output
        pm, mm, im, inm, om = matrices
        ordered = (pm, im, mm, inm, om)
        values = [BrainfuckStark._matrix_values(m, t.base_width) for m, t in zip(ordered, self.tables)]
        if any(v is None for v in values):
            return None
        if proof_stream is None:
            proof_stream = ProofStream()
        lib, stream = _lib.load(), current_stream()
        xf, n = self.xfield, self.fri.domain.length
        transcript = BrainfuckStark._native_transcript(proof_stream, xf, refuse_loaded=True)
        if transcript is None:
            return None
        t_begin = time.perf_counter()
        for table, matrix in zip(self.tables, ordered):
            table.matrix = matrix
        for table, v in zip(self.tables[3:], values[3:]):                       # io_table.py:17-21: length and height follow the symbols
            table.length = v.shape[0]
            table.height = v.shape[0] + table._padding_length(v.shape[0])
        for table, v in zip(self.tables[:3], values[:3]):
            if v.shape[0] + table._padding_length(v.shape[0]) != table.height:
                return None                                                     # (the Python path raises where the reference would)
        rnd, keep = self._native_randomness(n)          # (`keep` lives until this call returns)
        params = _lib.StarkParams(n.bit_length() - 1, self.expansion_factor, self.num_colinearity_checks, self.security_level,
                                  self.fri.domain.offset.value, self.fri.domain.omega.value, self.max_degree,
                                  (_u64 * 3)(*[t.height for t in self.tables[:3]]))
        tabs = (_lib.StarkTableIn * 5)()
        for slot, v in zip(tabs, values):
            slot.values, slot.rows, slot.row_stride = (v.ctypes.data if v.shape[0] else None), v.shape[0], (v.shape[1] if v.shape[0] else 0)
        session = BrainfuckStark._native_session()
        if not self._default_fri:          # (holds for the proof the next bfs_stark_commit starts)
            _lib.check(lib.bfs_stark_session_set_fri(session, self.fri._log2_folding, int(self.fri.coset_leaves), self.fri.grinding_bits))
        before = transcript.num_objects()
        out_ch, out_scan, out_io = (_u64 * 33)(), (_u64 * 27)(), (_u64 * 6)()
        ms_a, ms_b = (ctypes.c_double * 5)(), (ctypes.c_double * 5)()
        try:
            _lib.check(lib.bfs_stark_commit(session, transcript.handle, ctypes.byref(params), tabs, ctypes.byref(rnd), out_ch, out_scan, out_io,
                                            ms_a, stream))
            t_commit = time.perf_counter()
            # ---- while the GPU extends the extension columns: terminals, their objects, degree bounds
            challenges, terminals, terminal_objects = self._adopt_commit_reply(out_ch, out_scan, out_io, values[0][:, 2])
            transcript.scan(terminal_objects)
            handles = (_u64 * 5)(*[transcript.to_native(t) for t in terminal_objects])
            quotient_degree_bounds = self._quotient_degree_bounds(challenges, terminals, cached=True)
            shifts = self._layout.shifts(quotient_degree_bounds)
            unit_distances = self._layout.unit_distances(n)
            dist = (_u64 * (1 + len(unit_distances)))(0, *unit_distances)
            out_idx, out_top = (_u64 * max(self.security_level, 1))(), (_u64 * max(self.num_colinearity_checks, 1))()
            wseed = ctypes.create_string_buffer(32)
            t_host = time.perf_counter()
            _lib.check(lib.bfs_stark_finish(session, transcript.handle, handles, (_u64 * 15)(*[v for t in terminals for v in t]),
                                            (_u64 * len(shifts))(*shifts), len(shifts), transcript._field_id(BrainfuckStark.field), dist, len(dist),
                                            out_idx, wseed, out_top, ms_b, stream))
        except Exception:
            proof_stream._cached = None          # native code may have appended objects the Python list does not have
            raise
        proof_stream._adopt_lazy(transcript, before, transcript.num_objects(), xf)
        t_finish = time.perf_counter()
        proof = proof_stream.serialize()
        self._last = {"challenges": challenges, "terminals": terminals, "indices": [int(v) for v in out_idx[:self.security_level]],
                      "weights_seed": wseed.raw, "quotient_degree_bounds": quotient_degree_bounds}
        self.timing = {"host_prepare": t_commit - t_begin - sum(ms_a) * 1e-3, "pad": ms_a[0] * 1e-3, "randomizer": 0.0, "base_lde": ms_a[1] * 1e-3,
                       "base_tree": ms_a[2] * 1e-3, "extend": ms_a[3] * 1e-3, "ext_lde": ms_a[4] * 1e-3, "host_between_calls": t_host - t_commit,
                       "ext_tree": ms_b[0] * 1e-3, "quotients": 0.0, "combination": ms_b[1] * 1e-3, "combination_tree": ms_b[2] * 1e-3,
                       "openings": ms_b[3] * 1e-3, "fri": ms_b[4] * 1e-3 + (t_finish - t_host - sum(ms_b) * 1e-3),
                       "serialize": time.perf_counter() - t_finish}
        return proof

    _bounds_cache = {}

    def _quotient_degree_bounds(self, challenges, terminals, exact_terminals=False, cached=False):
        """all quotient degree bounds of a proof (:203-221): Table.all_quotient_degree_bounds of every table, then the permutation arguments.
        exact_terminals, for verify(): the challenges are Fiat-Shamir outputs, the terminals are the PROVER's, chosen after it has seen the
        challenges.  A terminal made from them (the product of two challenges, say) can cancel a monomial of a terminal constraint while
        looking as sampled as any other value; the reference expands symbolically every time and would then shift that quotient by a
        different amount than the generic bounds say.  So the terminal constraints -- the only ones the terminals enter -- take the exact
        expansion there (nine small constraints, ~50 us); boundary and transition bounds depend on the challenges alone.
        cached, for the native prover: remembered per SHAPE of the inputs.  Which monomials of the composed constraints survive depends
        on the numeric challenges, terminals and parameters only through cancellations (table.py: _degree_bounds); values that look
        sampled (more than 32 significant bits) behave generically except with negligible probability, small ones (zero, the `iota^0 = 1`
        of an IO table without padding, a crafted test value) are part of the key as they are.  The per-table code draws the same line but
        falls back to the exact expansion whenever ANY value is small -- every proof of a program without input does, 160 us of host time."""
        key = None
        if cached:
            assert not exact_terminals
            values = list(challenges) + list(terminals) + [p for t in self.tables for p in t.air_params(challenges)]
            sampled = [v for v in values if v[0] >> 32 or v[1] or v[2]]
            if len(set(sampled)) == len(sampled):
                key = (tuple(t.height for t in self.tables), tuple(t.length for t in self.tables[3:]),
                       tuple("s" if (v[0] >> 32 or v[1] or v[2]) else tuple(v) for v in values))
                hit = BrainfuckStark._bounds_cache.get(key)
                if hit is not None:
                    return list(hit)
        out = [b for table in self.tables for b in table.all_quotient_degree_bounds(challenges, terminals, exact_terminals=exact_terminals)]
        out += [pa.quotient_degree_bound() for pa in self.permutation_arguments]
        if key is not None:
            if len(BrainfuckStark._bounds_cache) > 1024:
                BrainfuckStark._bounds_cache.clear()
            BrainfuckStark._bounds_cache[key] = tuple(out)
        return out

    def _terminal_objects(self, terminals):
        """the five terminals as the OBJECTS the reference pushes (:223-224).  The input and output evaluations both start from ONE zero
        object (processor_table.py:340-347) and stay that object when the program never reads / writes; pickle then writes the second
        one as a back-reference.  The running evaluations are sums `evaluation * challenge + lift(symbol)`; the first one is `zero +
        lift(symbol)`, which returns the lifted symbol's polynomial, and from then on the left operand's coefficients --
        BaseFieldElements of the VM's BaseField instance (vm.py:70), not of the extension field's own -- decide the field of every
        result (processor_table.py:390-404, univariate.py:23-35): pickle writes that third BaseField instance out."""
        xf = self.xfield
        terminal_objects = [xf.from_limbs(t) for t in terminals]
        for k, identity in zip((2, 3), self.processor_table.evaluation_terminal_identities):
            limbs = list(terminals[k])
            while limbs and limbs[-1] == 0:
                limbs.pop()
            if limbs and identity is not None and identity[0] == "object":
                terminal_objects[k] = ExtensionFieldElement(Polynomial([identity[1]]), xf)
            elif limbs:
                base = identity[1] if identity is not None else VirtualMachine.field
                terminal_objects[k] = ExtensionFieldElement(Polynomial([BaseFieldElement(v, base) for v in limbs]), xf)
        if not any(terminals[2]) and not any(terminals[3]):
            terminal_objects[3] = terminal_objects[2]
        return terminal_objects

    # ---- the Python stage driver: one method per stage, named after the `timing` key the stage ends on, over one per-proof record `p`
    def _prove(self, program, processor_matrix, memory_matrix, instruction_matrix, input_matrix, output_matrix, proof_stream=None):
        assert len(processor_matrix) + len(program) == len(instruction_matrix)
        proof = self._prove_native(program, (processor_matrix, memory_matrix, instruction_matrix, input_matrix, output_matrix), proof_stream)
        if proof is not None:
            return proof
        # the per-proof record (nothing in it refers to this object): the matrices in the order of self.tables and what else is given; the stages
        # add draw, randomizer_polynomial, randomizer_codeword, prepared_extension, rows (the _RowBuilder), base_tree, challenges, terminals,
        # extension_tree, weights_seed, combination, combination_tree, indices, unit_distances, known (the opened combination leaves), proof
        p = SimpleNamespace(matrices=(processor_matrix, instruction_matrix, memory_matrix, input_matrix, output_matrix), proof_stream=proof_stream,
                            domain=self.fri.domain, n=self.fri.domain.length, stream=current_stream(), quotient_degree_bounds=None, quotient_buffers=[])
        return self._run_stages(p, (("pad", self._stage_pad),           # (includes the randomizer's GPU time where it outlasts the padding)
                                    ("randomizer", None), ("base_lde", self._stage_base_lde), ("base_tree", self._stage_base_tree),
                                    ("extend", self._stage_extend), ("ext_lde", self._stage_ext_lde), ("ext_tree", self._stage_ext_tree),
                                    ("quotients", self._stage_quotients), ("combination", self._stage_combination),
                                    ("combination_tree", self._stage_combination_tree), ("openings", self._stage_openings),
                                    ("fri", self._stage_fri), ("serialize", self._stage_serialize)))

    def _run_stages(self, p, stages):
        """the stage loop of both protocols: stages = (timing key, function of the record `p` or None for a key without a stage), run in
        order; `timing` gets the keys in that order, split by stage on the GPU too where stage_timing is set.  -> p.proof"""
        self.timing, mark = {}, time.perf_counter()
        for name, stage in stages:
            if stage is not None:
                stage(p)
            if self.stage_timing:
                synchronize(p.stream)
            now = time.perf_counter()
            self.timing[name], mark = now - mark, now
        return p.proof

    def _random_source(self):
        """where a proof draws from: the module's urandom, read now (tests patch it), or this context's shared stream (randomness.override)"""
        return random_source(urandom)

    _canonical_limbs = staticmethod(_canonical_limbs)          # (deep_stark's verifier reads proofs through the same rule)

    def _stage_pad(self, p):
        """randomizer polynomial and codeword (:162-167) -- queued FIRST: padding (:143-148) is host work that draws no randomness, so the
        GPU expands and transforms the randomizer while the host pads (the order of the random draws is the reference's either way)"""
        xf, count = self.xfield, self.max_degree + 1
        p.draw = self._random_source()
        seed, blob = _seed_or_stream(p.draw, 3 * 9 * count)      # `count` draws of 27 bytes
        if seed is not None:
            p.randomizer_polynomial = XArray.empty(count, xf)
            _lib.check(_lib.load().bfs_xfe_sample_fill(seed, p.randomizer_polynomial.ptr, count, count, p.stream))
        else:
            p.randomizer_polynomial = XArray.from_numpy(sample_ext_many(blob, count, 9), xf)
        p.randomizer_codeword = p.domain.xevaluate(p.randomizer_polynomial, xf, as_array=True)
        self._pad_tables(p)

    def _pad_tables(self, p):          # the matrices onto the tables, padded (host work, no randomness); the proof stream if none was given
        for table, matrix in zip(self.tables, p.matrices):
            table.matrix = matrix
        for table in (self.processor_table, self.memory_table, self.instruction_table, self.input_table, self.output_table):
            table.pad()                                                                      # :143-148
        if p.proof_stream is None:
            p.proof_stream = ProofStream()

    def _stage_base_lde(self, p):          # base codewords of all tables (:169-172)
        lde_tables(self.tables, p.domain)
        p.prepared_extension = prepare_extension(self.tables)      # host work (row masks) behind the transform that has just been queued

    def _stage_base_tree(self, p):          # one commitment to the zipped rows of randomizer and base codewords (:174-179)
        p.rows = _RowBuilder(self._layout, p.n, p.randomizer_codeword, BrainfuckStark.field, self.xfield)
        columns = [(p.randomizer_codeword.ptr, True, 0)] + [(address, False, 0) for _, _, address, _ in self._layout.device_columns(p.n, 0)]
        p.base_tree = self._zipped_tree(columns, p.n, p.rows.base_row)
        p.proof_stream.push(p.base_tree.root())

    def _stage_extend(self, p):          # challenges, initials, table extension, terminals (:181-192)
        p.challenges = tuple(BrainfuckStark._sample_weights(11, p.proof_stream.prover_fiat_shamir()))
        initials = [sample_ext(p.draw(3 * 8)) for _ in self.permutation_arguments]
        extend_tables_device(self.tables, p.challenges, initials, prepared=p.prepared_extension)   # prefix scans on the trace columns lde() left in HBM
        p.terminals = self.get_terminals()
        if self.check_air:              # the trace against the AIR it is about to be proven for, on the columns in HBM
            violations = [v for t in self.tables if t.length for v in t.air_violations(p.challenges, p.terminals)]
            if violations:
                raise AirViolationError(violations)

    def _stage_ext_lde(self, p):          # extension codewords (:194-195)
        lde_tables(self.tables, p.domain, extension=True)
        if not self.keep_intermediates:
            # the quotient degree bounds (:203-221) are host work on challenges and terminals: done here, while the GPU runs the coset
            # transform of the extension columns that lde_tables has just queued
            p.quotient_degree_bounds = self._quotient_degree_bounds(p.challenges, p.terminals)

    def _stage_ext_tree(self, p):          # the commitment to the zipped rows of the extension codewords (:197-201)
        p.rows.share([m for t in self.tables for m in t.ext_sharing_moduli(p.n)])
        columns = [(address, True, 0) for _, _, address, _ in self._layout.device_columns(p.n, 1)]
        p.extension_tree = self._zipped_tree(columns, p.n, p.rows.ext_row)
        p.proof_stream.push(p.extension_tree.root())

    def _stage_quotients(self, p):
        """quotients (:203-221).  keep_intermediates (tests): the quotient codewords are written out and summed by bfs_combination, as the
        reference does; otherwise they only ever exist in registers (bfs_air_combine).  Same field elements either way."""
        if not self.keep_intermediates:
            return
        domain = p.domain
        p.quotient_buffers = [(table.all_quotients(domain, None, p.challenges, p.terminals), table.num_quotients()) for table in self.tables]
        p.quotient_buffers += [(pa.quotient(domain), 1) for pa in self.permutation_arguments]
        p.quotient_degree_bounds = self._quotient_degree_bounds(p.challenges, p.terminals)
        from . import debug_checks
        if debug_checks.enabled():
            debug_checks.check_prover(self, p.quotient_buffers, self._layout.column_degree_bounds(), p.quotient_degree_bounds)

    def _stage_combination(self, p):          # terminals (:223-224), weights (:226-243) and the non-linear combination (:245-298)
        for t in self._terminal_objects(p.terminals):
            p.proof_stream.push(t)
        p.weights_seed = p.proof_stream.prover_fiat_shamir()
        weight_array = BrainfuckStark._sample_weights(self._layout.weight_count, p.weights_seed, as_array=True)
        weight0 = tuple(int(v) for v in weight_array[0])
        # terms in the order of the reference's `terms` list (_TermLayout); each is shifted to the common degree bound.  One row of seven
        # words per term (bfs_comb_weight).
        shifts = self._layout.shifts(p.quotient_degree_bounds)
        assert 1 + 2 * len(shifts) == len(weight_array)
        terms = np.empty((len(shifts), 7), dtype=np.uint64)
        terms[:, 0:3], terms[:, 3:6], terms[:, 6] = weight_array[1::2], weight_array[2::2], shifts
        if self._shift_tweak is not None:
            terms[:, 6] = self._shift_tweak(terms[:, 6])
        p.combination = XArray.empty(p.n, self.xfield)
        if self.keep_intermediates:
            self._combine_written_out(p, terms, weight0)
        else:
            self._combine_fused(p, terms, weight0)
            BrainfuckStark._release(p.randomizer_polynomial, *[buf for buf, _ in p.quotient_buffers])
            p.quotient_buffers = []

    @staticmethod
    def _term(terms, s):
        return tuple(int(v) for v in terms[s, 0:3]), tuple(int(v) for v in terms[s, 3:6]), int(terms[s, 6])

    def _combine_written_out(self, p, terms, weight0):
        """bfs_combination: one weighted sum over the column codewords and the quotient codewords that _stage_quotients wrote out"""
        n, domain = p.n, p.domain
        sources = [(address, ext) for ext in (0, 1) for _, _, address, _ in self._layout.device_columns(n, ext)]
        sources += [(buf.ptr + 8 * 3 * q * n, 1) for buf, count in p.quotient_buffers for q in range(count)]
        assert len(sources) == len(terms)
        srcs = (_lib.CombSource * len(sources))()
        for s, (ptr, is_ext) in enumerate(sources):
            wa, wb, shift = self._term(terms, s)
            srcs[s].ptr, srcs[s].is_ext, srcs[s].shift = ptr, is_ext, shift
            srcs[s].wa, srcs[s].wb = (_u64 * 3)(*wa), (_u64 * 3)(*wb)
        _lib.check(_lib.load().bfs_combination(srcs, len(sources), p.randomizer_codeword.ptr, (_u64 * 3)(*weight0), p.combination.ptr,
                                               n.bit_length() - 1, domain.offset.value, domain.omega.value, p.stream))

    def _combine_fused(self, p, terms, weight0):
        """bfs_air_combine: every table's columns and quotients folded into the accumulator, the quotients never written out.
        A cooperative proof (cooperate()): the stage is pointwise, every rank holds all codewords (a row's neighbour at unit_distance
        comes from the rank's own copy), so each rank does its own rows and the ranks all-gather the combination.
        _row_windows (tests): the same row-window entry points on one GPU, the domain cut into arbitrary pieces."""
        n, domain, layout = p.n, p.domain, self._layout
        rows = None
        if self._cooperation is not None:
            from .shard import row_range
            rows = row_range(n, self._cooperation[0], self._cooperation[1])
        windows = [rows]
        if rows is None and self._row_windows is not None:
            windows = list(self._row_windows)
            # run in the order given (every window initialises its own rows of the accumulator): any order of a tiling
            ends = [first + count for first, count in sorted(windows)]
            assert [first for first, _ in sorted(windows)] == [0] + ends[:-1] and ends[-1] == n, "the windows must tile the domain"
        for window in windows:
            inverse_buffer, inverses = zerofier_inverses(self.tables, domain, rows=window)      # all zerofier denominators, one inversion per point
            for k, t in enumerate(self.tables):
                mine = np.concatenate([terms[layout.base[k]], terms[layout.ext[k]], terms[layout.quot[k]]])
                t.combine_into(domain, p.challenges, p.terminals, mine, p.combination, randomizer=p.randomizer_codeword if k == 0 else None,
                               randomizer_weight=weight0, inverses=inverses[t], rows=window)
            for j, pa in enumerate(self.permutation_arguments):
                pa.combine_into(domain, self._term(terms, layout.first_argument + j), p.combination, inv_x_minus_1=inverses[self.tables[0]][0],
                                rows=window)
            inverse_buffer.free()
        if rows is not None:
            from .shard import all_gather_rows
            world_size, rank, group, device = self._cooperation
            all_gather_rows(p.combination.ptr, n, 3, p.combination.stride, world_size, rank, group=group, device=device, stream=p.stream)

    def _stage_combination_tree(self, p):
        """commitment to the combination codeword (:300-302).  (GPU work: 2^22 extension leaves are 1.1 ms)"""
        if self.fri.coset_leaves:          # one leaf per folding coset: the tree FRI's round 0 commits to in this form
            p.combination_tree = CosetMerkle(p.combination, self.fri.folding_factor)
        else:
            p.combination_tree = Merkle(p.combination)
        p.proof_stream.push(p.combination_tree.root())

    def _stage_openings(self, p):          # the opened rows and combination leaves (:304-333)
        p.indices = BrainfuckStark.sample_indices(self.security_level, p.proof_stream.prover_fiat_shamir(), p.n)
        p.unit_distances = self._layout.unit_distances(p.n)
        p.known = self._openings_native(p)
        if p.known is None:
            p.known = self._openings_python(p)
        if not self.keep_intermediates:
            BrainfuckStark._release(p.base_tree, p.extension_tree, p.randomizer_codeword, *self.tables)
            p.base_tree = p.extension_tree = None

    def _stage_fri(self, p):
        """low-degree test of the combination codeword (:335-336); round 0 commits to the combination tree that was just built"""
        self.fri.prove(p.combination, p.proof_stream, known_leafs=p.known or None, round0_tree=p.combination_tree)
        self._last = {"challenges": p.challenges, "terminals": p.terminals, "indices": p.indices, "weights_seed": p.weights_seed,
                      "quotient_degree_bounds": p.quotient_degree_bounds}
        if self.keep_intermediates:
            self._last.update({"base_tree": p.base_tree, "extension_tree": p.extension_tree, "combination_tree": p.combination_tree,
                               "quotient_buffers": p.quotient_buffers, "combination": p.combination, "randomizer_codeword": p.randomizer_codeword})
        else:
            BrainfuckStark._release(p.combination, p.combination_tree)

    def _stage_serialize(self, p):
        p.proof = p.proof_stream.serialize()

    # ---- proving by out-of-domain openings: the second protocol, deep_stark.py; these methods hand over to it
    def deep_shape(self, segmented=False, zero_knowledge=False):
        """The domains of prove_deep / verify_deep as the namespace L, S, s, n, w, fri, domain, working_domain that deep_segmented_shape()
        describes; segmented=True is that shape.  The unsegmented mode is its case of ONE segment, and both run the same code on their
        shape: the constructor makes max_degree + 1 a power of two and self.fri's domain expansion_factor times as long, so
        L = S = max_degree + 1, s = 1, n = w = self.fri.domain.length with fri = self.fri and domain = working_domain = self.fri.domain
        (these objects: no Fri is made, nothing is refused) say what that mode does -- no decimation (w = n), H on every
        expansion_factor-th point (w / S), its S coefficients the one segment, and the verifier's Horner loop in z^L over one value H(z).

        The namespace also carries k, m, L0, randomizer, hiding -- 0, 0, L, False, False unless zero_knowledge ("Zero-knowledge
        openings").  With t the number of colinearity checks, zero_knowledge=True makes them
          k = 2 t + 6   blinding coefficients per trace column: f + (X^h - 1) r has h + k coefficients;
          S  the power of two above the largest transition quotient degree bound for such interpolants (the constructor's analysis);
          L  (segmented) the power of two >= the largest h + k; (unsegmented) S;
          m = t + 1, L0 = L - m, s = ceil(S / L0) blinded segments of at most L coefficients (segmented); m = 0, L0 = L, s = 1 otherwise;
          randomizer = hiding = True: C2 carries a uniform masking polynomial of L coefficients, the three row trees are salted.
        s + 1 > 16 or m > L0 is refused with the ValueError of deep_segmented_shape."""
        return deep_stark.make_shape(self, segmented, zero_knowledge)

    def deep_segmented_shape(self):
        """The domains of the segmented mode of prove_deep / verify_deep ("Segmented composition"), from public data alone.
        With e the expansion factor:
          L  the power of two >= the largest coefficient count of a trace interpolant (Table.transform_coefficients), at least 1;
          S  max(max_degree + 1, L): the coefficients of H, as in the unsegmented mode;
          s  S // L segments H_i of L coefficients each, H(x) = sum_i x^(i L) H_i(x);
          n  e L, the length of the commitment and FRI domain offset * omega_n^i (offset the field's generator, as self.fri's);
          w  max(n, S), the length of the working domain the trace is extended to: the commitment domain is every (w / n)-th of its
             points, the points H is computed on every (w / S)-th.
        s > 16 (pcs.MAX_EXT_COLUMNS) is refused with a ValueError.  It cannot arise with this AIR at e >= 4: a table's transition
        degree is at most 10 h_t + 1 (the processor's), so S <= 16 h for the tallest table's h, while L >= 2 h holds its h + 1
        coefficients -- s <= 8 (and >= 2: the memory table's 2 h_t + 1).
        -> namespace L, S, s, n, w, fri (a second Fri over the n points with the constructor's modes, made on first use and kept),
        domain (its domain), working_domain"""
        return self.deep_shape(True)

    def prove_deep(self, program, processor_matrix, memory_matrix, instruction_matrix, input_matrix, output_matrix, proof_stream=None,
                   segmented=False, zero_knowledge=False, secret_input=False):
        """A proof of the same claim as prove()'s in the form current STARKs use (DEEP-ALI): C0 commits to the 16 base columns, C1 -- after
        the 11 challenges -- to the 9 extension columns, C2 -- after the terminals and one weight per quotient -- to the composition
        polynomial H = sum beta_q quotient_q, computed on every expansion_factor-th point of the domain (bfsc_air_compose) and
        interpolated to N / expansion_factor coefficients; then z is drawn and one `open_rounds` opens every table's columns at z and at
        its next row z * omicron, and H at z.  verify_deep() checks the opening and the one identity that ties H(z) to the opened rows.
        The Fri modes of the constructor apply as they are.  Returns the proof bytes; for a false trace too (verify_deep refuses them).

        segmented=True (deep_segmented_shape): the three commitments and the FRI proof live on a domain of expansion_factor * L points, L
        the power of two that holds a trace interpolant, instead of expansion_factor * (max_degree + 1); the trace is extended to the
        working domain of max(that, max_degree + 1) points, on which H is computed as before; C0 and C1 commit to every (w / n)-th word
        of the codewords (bfsg_decimate_rows; the codewords as they lie where w = n), and C2 to the s = (max_degree + 1) / L segments
        H_i of H(x) = sum_i x^(i L) H_i(x), all opened at z.  The random draws and the order of the stream are the unsegmented mode's;
        the bytes are not, and each verifier refuses the other mode's proofs.

        zero_knowledge=False is NOT zero-knowledge, segmented or not: the commitments are not hiding (pcs.py: unsalted row trees, plain
        values in the proof) and no randomizer polynomial is mixed in; the one trace randomizer per column only keeps the interpolants'
        shape of prove().

        zero_knowledge=True ("Zero-knowledge openings"; deep_shape gives the numbers) hides the trace in either mode: every
        column of a table with rows is blinded by (X^h - 1) r with k = 2 t + 6 uniform coefficients (bfsz_poly_blind) -- as many as the
        base-field functionals one proof reveals of it: t opened rows, their t next rows through H, two openings in F_p^3 --, the segments
        of H are blinded so that they still sum to H (bfsz_split_blind, m = t + 1 coefficients each), C2 also commits to a uniform
        polynomial R of L coefficients that is opened at z and masks the DEEP quotient with everything FRI shows of it, and the three row
        trees are salted (pcs.PolynomialCommitment(hiding=True)).  Not hidden: the terminals (pushed in the clear, as prove() does) and
        the heights; the blinding draws carry the bias of the reference's 9-bytes-mod-p sampling.  The bytes differ from the other modes',
        and each of the four verifiers refuses the other three kinds of proof.

        secret_input=True ("Secret input"; needs zero_knowledge=True and an object made with input_symbols="", else ValueError)
        proves another claim: there IS an input on which `program` runs running_time cycles over memory_length memory rows and writes
        output_symbols.  The matrices are those of a run on that input; the input matrix given is dropped -- the input table has no rows
        --, the input evaluation terminal is not sent (four terminals; the kernels' terminal vector holds zero in its slot) and the
        weight of the processor table's terminal constraint against it is zero (deep_stark.dropped_weight).  Everything else is the
        zero-knowledge mode's; each verifier without secret_input refuses such a proof, and verify_deep(secret_input=True) the others'."""
        return deep_stark.prove(self, program, (processor_matrix, memory_matrix, instruction_matrix, input_matrix, output_matrix), proof_stream,
                                self.deep_shape(segmented, zero_knowledge), secret_input=secret_input)

    def deep_weight_count(self):
        """one weight per quotient: the tables' (boundary, transition, terminal within a table), then the permutation arguments'"""
        return sum(t.num_quotients() for t in self.tables) + len(self.permutation_arguments)

    def compose_into(self, out, log_step, weights, challenges, terminals, domain=None):
        """H on every 2^log_step-th point of `domain` -- the FRI domain unless given; the one the tables' codewords lie on -- into `out`
        (XArray of N >> log_step elements): bfsc_air_compose per table with rows, bfsc_difference_compose per permutation argument; the
        first call writes, the others add.  weights: (deep_weight_count(), 3) uint64; weights of a table without rows are skipped."""
        deep_stark.compose_into(self, out, log_step, weights, challenges, terminals, domain)

    def verify_deep(self, proof, segmented=False, zero_knowledge=False, secret_input=False):
        """the verifier of prove_deep -- host code only (Python ints, hashlib, Fri.verify): the terminals against the public input, output
        and program; the opening of the 26 columns at the plan's points for the values the prover claims (read_rounds); every value of a
        table without rows zero; and
            sum_t sum_q beta_{t,q} constraint_{t,q}(cur_t, nxt_t) Z_kind(z) + sum_j beta_j (lhs_j(z) - rhs_j(z)) / (z - 1) = H(z)
        with Z the zerofier factors of csrc/air.hip: 1 / (z - 1), (z - omicron^-1) / (z^h - 1), 1 / (z - omicron^-1).
        False with one printed line for every refusal, a malformed stream included; raises nothing.
        segmented=True verifies prove_deep(segmented=True)'s proofs: the opening is read over the Fri of deep_segmented_shape(), the last
        group holds the s segments, and the right-hand side is H(z) = sum_i z^(i L) H_i(z).  A proof of the other mode has another
        shape (widths, domain length) and is refused by the opening's reader like any stream that is not this mode's.
        zero_knowledge=True verifies prove_deep(zero_knowledge=True)'s proofs of the same `segmented`: the roots and paths are salted
        ((salt, path) behind each opened row, checked with SaltedMerkle.verify), the last group holds the s blinded segments and the
        masking polynomial's value, which the opening alone uses, and the right-hand side is H(z) = sum_j z^(j L0) H_j'(z).  A proof of
        another combination differs in width, salt or path shape and is refused.
        secret_input=True verifies prove_deep(secret_input=True)'s proofs on an object made with input_symbols="" (ValueError otherwise, and
        without zero_knowledge=True): four terminals are read, the input evaluation argument is not compared, the dropped constraint's
        weight is zero; the output and program terminals are checked as ever.  A proof with five terminals is refused, and a secret-input
        proof by every verifier without secret_input: the object behind the last terminal is not what either expects there."""
        # (what deep_shape and the secret-input check raise is about this object and this call, not about the proof)
        return deep_stark.verify(self, proof, self.deep_shape(segmented, zero_knowledge), secret_input=secret_input)

    # ------------------------------------------------------------------------------------------------------------
    def check_trace(self, processor_matrix, memory_matrix, instruction_matrix, input_matrix, output_matrix, challenges=None, initials=None,
                    secret_input=False):
        """Which constraints an execution trace breaks, on the GPU: a list of AirViolation, empty for an honest trace.  The base AIR of
        every table on the matrices as given (test_vm.py::test_air); with challenges (11 triples) and initials (2 triples) also the
        full AIR on padded, extended copies, each table against its own terminals, and then what no single table's AIR sees -- the
        terminals of the two permutation arguments (processor against instruction / memory table) and the input, output and
        program evaluation terminals against this stark's input_symbols, output_symbols and program (what verify() checks).
        Those come back as kind "permutation" (index 0 instruction, 1 memory) / "evaluation" (0 input, 1 output, 2 program) with
        first_row None; an input or output MATRIX that does not hold the symbols the processor read or wrote comes back the same way
        under the table name "input" / "output".  The caller's matrices are left as they are.
        secret_input=True (the claim of prove_deep(secret_input=True): the input is not public) leaves out the two checks that name the
        input -- the processor's input evaluation terminal against input_symbols, and the input matrix against what the processor read."""
        import copy
        matrices = {0: processor_matrix, 1: instruction_matrix, 2: memory_matrix, 3: input_matrix, 4: output_matrix}
        tables = []
        for t in self.tables:
            c = copy.copy(t)
            c.matrix = matrices[t.table_index]
            c._array_for = None
            c.length = len(c.matrix)              # (the matrices given, not the claim this stark was made for)
            c.height = c.roundup_npo2(c.length)
            c.ext_columns = c._base_device = c._ext_device = c.base_codewords = c.ext_codewords = None
            tables.append(c)
        violations = [v for t in tables for v in t.air_violations()]
        if challenges is None:
            return violations
        challenges = [tuple(int(x) for x in (c.limbs() if hasattr(c, "limbs") else c)) for c in challenges]
        initials = [tuple(int(x) for x in (c.limbs() if hasattr(c, "limbs") else c)) for c in initials]
        for t in tables:
            t.pad()
        for t in tables:
            t.extend(challenges, initials)
        pt, it, mt, inp, outp = tables
        own = [pt.instruction_permutation_terminal, pt.memory_permutation_terminal, pt.input_evaluation_terminal,
               pt.output_evaluation_terminal, it.evaluation_terminal]
        for t in tables:
            terminals = list(own)
            if t is it:
                terminals[0] = it.permutation_terminal
            elif t is mt:
                terminals[1] = mt.permutation_terminal
            elif t is inp:
                terminals[2] = inp.evaluation_terminal
            elif t is outp:
                terminals[3] = outp.evaluation_terminal
            if t.length:
                violations += t.air_violations(challenges, terminals)
        pairs = [("processor", "permutation", 0, pt.instruction_permutation_terminal, it.permutation_terminal),
                 ("processor", "permutation", 1, pt.memory_permutation_terminal, mt.permutation_terminal)]
        for k, (name, terminal) in enumerate((("processor", pt.input_evaluation_terminal), ("processor", pt.output_evaluation_terminal),
                                              ("instruction", it.evaluation_terminal))):
            pairs.append((name, "evaluation", k, terminal, self.evaluation_arguments[k].compute_terminal(challenges)))
        # ... and the input / output table against the processor's running evaluations: prove() sends the processor's terminals, and the
        # IO tables' terminal constraints are taken against those
        pairs += [("input", "evaluation", 0, inp.evaluation_terminal, pt.input_evaluation_terminal),
                  ("output", "evaluation", 1, outp.evaluation_terminal, pt.output_evaluation_terminal)]
        if secret_input:
            pairs = [pair for pair in pairs if pair[1:3] != ("evaluation", 0)]
        violations += [AirViolation(name, kind, k, None, 1) for name, kind, k, lhs, rhs in pairs if tuple(lhs) != tuple(rhs)]
        return violations

    def verify(self, proof, proof_stream=None):
        """brainfuck_stark.py:343-579 -- host only, like the reference's verifier: Merkle paths of the opened rows, the
        non-linear combination recomputed from the opened rows (constraints evaluated through air.evaluate), FRI, and the
        terminals against the public input, output and program."""
        if proof_stream is None and self.native_stages:
            verdict = self._verify_native(proof)
            if verdict is not None:
                return verdict
        if proof_stream is None:
            proof_stream = ProofStream()
        proof_stream = proof_stream.deserialize(proof)
        # leaf preimages (pickle.dumps of an opened row / element) come from the native copy of the stream while this call runs
        token = leaf_pickle_source.set(proof_stream.pickle_of) if hasattr(proof_stream, "pickle_of") else None
        try:
            return self._verify_stream(proof_stream)
        except _MalformedProof:
            return False
        finally:
            if token is not None:
                leaf_pickle_source.reset(token)

    def _verify_native(self, proof):
        """verify() on the native object graph of the proof (csrc/verifier.cpp: bfs_stark_verify_begin / _finish): the same checks in the same
        order as _verify_stream / Fri.verify below, without a Python object per pulled item.  Returns True / False, raises the reference's
        AssertionError -- or returns None when this route does not apply (the bytes are not something the native reader takes, or the stream
        holds an object the native checks do not model): the Python verifier below then decides, as the reference would."""
        if os.environ.get("BFS_NATIVE_VERIFY", "1") == "0":
            return None
        from .ip import NativeTranscript
        try:
            data = bytes(proof)
        except TypeError:
            return None
        t = NativeTranscript.from_bytes(data)
        if t is None:
            return None
        lib, n = _lib.load(), self.fri.domain.length
        unit_distances = self._layout.unit_distances(n)
        if len(unit_distances) > 8:
            return None
        words = (_u64 * max(len(self.program), 1))(*[w.value if hasattr(w, "value") else int(w) for w in self.program])
        ins = (_u64 * max(len(self.input_symbols), 1))(*[ord(c) for c in self.input_symbols])
        outs = (_u64 * max(len(self.output_symbols), 1))(*[ord(c) for c in self.output_symbols])
        params = _lib.StarkVerifyParams()
        params.log_n, params.expansion_factor = n.bit_length() - 1, self.expansion_factor
        params.num_colinearity_checks, params.security_level = self.num_colinearity_checks, self.security_level
        params.offset, params.omega = self.fri.domain.offset.value, self.fri.domain.omega.value
        params.heights = (_u64 * 5)(*[t_.height for t_ in self.tables])
        params.lengths = (_u64 * 5)(*[t_.length for t_ in self.tables])
        params.omicrons = (_u64 * 5)(*[t_.omicron.value for t_ in self.tables])
        params.num_distances, params.distances = len(unit_distances), (_u64 * 8)(*(unit_distances + [0] * (8 - len(unit_distances))))
        params.program, params.program_len = ctypes.addressof(words), len(self.program)
        params.input, params.n_input = ctypes.addressof(ins), len(self.input_symbols)
        params.output, params.n_output = ctypes.addressof(outs), len(self.output_symbols)
        out_ch, out_tm, verdict = (_u64 * 33)(), (_u64 * 15)(), ctypes.c_int(3)
        _lib.check(lib.bfs_stark_verify_begin(t.handle, ctypes.byref(params), out_ch, out_tm, ctypes.byref(verdict)))

        def outcome():          # 1: accepted, 2: the reference's assertion, 3: this route does not apply, else refused
            if verdict.value == 2:
                raise AssertionError(lib.bfs_last_error().decode("utf-8", "replace"))
            return None if verdict.value == 3 else verdict.value == 1
        if verdict.value != 1:
            return outcome()
        challenges, terminals = tuple(_triples(out_ch, 11)), _triples(out_tm, 5)
        shifts = self._layout.shifts(self._quotient_degree_bounds(challenges, terminals, exact_terminals=True))
        if self._default_fri:
            _lib.check(lib.bfs_stark_verify_finish(t.handle, ctypes.byref(params), (_u64 * len(shifts))(*shifts), len(shifts), ctypes.byref(verdict)))
        else:
            _lib.check(lib.bfs_stark_verify_finish_fri(t.handle, ctypes.byref(params), (_u64 * len(shifts))(*shifts), len(shifts),
                                                       self.fri._log2_folding, int(self.fri.coset_leaves), self.fri.grinding_bits, ctypes.byref(verdict)))
        return outcome()

    # ---- the Python verifier, in the order of the reference's verify(): head, opened rows, per index the combination, tail
    def _verify_stream(self, proof_stream):
        head = self._verify_head(proof_stream)
        rows = self._verify_opened_rows(proof_stream, head)
        shifts = self._layout.shifts(self._quotient_degree_bounds(head.challenges, head.terminals, exact_terminals=True))
        weights_raw = head.weights.ctypes.data_as(ctypes.POINTER(_u64))
        for index in head.indices:
            terms = self._combination_terms(head, rows, index, shifts)
            assert len(terms) == len(head.weights), f"length of terms ({len(terms)}) must be equal to length of weights ({len(head.weights)})"
            flat = (_u64 * (3 * len(terms)))(*[v for t in terms for v in t])          # bfs_xfe_inner_product: 303 products natively
            got = (_u64 * 3)()
            _lib.check(_lib.load().bfs_xfe_inner_product(weights_raw, flat, len(terms), got))
            inner_product = (got[0], got[1], got[2])
            combination_leaf = proof_stream.pull()
            combination_path = proof_stream.pull()
            if self.fri.coset_leaves:
                # the opened leaf is the coset tuple of leaf c = index mod q: a extension elements, authenticated by log2 q digests;
                # the combination value at `index` is its element number index // q
                a, q = self.fri.folding_factor, self.fri.domain.length // self.fri.folding_factor
                if not (isinstance(combination_leaf, tuple) and len(combination_leaf) == a and all(hasattr(e, "limbs") for e in combination_leaf)):
                    return False
                if not (isinstance(combination_path, list) and len(combination_path) == q.bit_length() - 1
                        and all(isinstance(node, (bytes, bytearray)) for node in combination_path)):
                    return False
                if not Merkle.verify(head.combination_root, index % q, combination_path, combination_leaf):
                    return False
                combination_leaf = combination_leaf[index // q]
            elif not Merkle.verify(head.combination_root, index, combination_path, combination_leaf):
                return False
            # brainfuck_stark.py:567 compares the leaf OBJECT with the inner product (coefficient values as stored, algebra.py:36):
            # a leaf whose coefficients are not canonical residues is unequal there, and here
            if not hasattr(combination_leaf, "limbs") or tuple(combination_leaf.limbs()) != inner_product:
                return False
        verdict = self.fri.verify(proof_stream, head.combination_root)
        for ea in self.evaluation_arguments:
            verdict = verdict and tuple(ea.select_terminal(head.stored_terminals)) == tuple(ea.compute_terminal(head.challenges))
        return bool(verdict)

    def _verify_head(self, proof_stream):
        """everything up to the opened rows: roots, challenges, terminals, weights, indices (:357-413)"""
        head = SimpleNamespace(base_root=proof_stream.pull())
        head.challenges = challenges = tuple(BrainfuckStark._sample_weights(11, proof_stream.verifier_fiat_shamir()))
        head.extension_root = proof_stream.pull()
        terminal_objects = [proof_stream.pull() for _ in range(5)]
        head.terminals = [_canonical_limbs(t) for t in terminal_objects]
        # ... and as STORED, for the three evaluation arguments at the end: the reference compares the pulled object with a computed
        # element through Polynomial.__eq__ / BaseFieldElement.__eq__, i.e. the coefficient values as they were pickled
        head.stored_terminals = stored = [tuple(t.limbs()) if hasattr(t, "limbs") else (t.value, 0, 0) for t in terminal_objects]
        # io_table.py:54-56, which the reference reaches through num_quotients below (brainfuck_stark.py:394-395): a non-empty input
        # (output) table against a terminal stored as all zeros raises there instead of ending in False; input table first.  NOT where
        # the claim's own symbols evaluate to zero too (a single symbol 0: `-+.`): such claims are proven and verified here, while the
        # reference's prover stops at that very assertion.
        for io, ea in zip((self.input_table, self.output_table), self.evaluation_arguments):
            if io.height != 0 and not any(stored[io.terminal_index]):
                assert not any(ea.compute_terminal(challenges)), "evaluation terminal for non-empty IOTable is zero but shouldn't be!"
        weights = BrainfuckStark._sample_weights(self._layout.weight_count, proof_stream.verifier_fiat_shamir(), as_array=True)
        head.weights = np.ascontiguousarray(weights, dtype=np.uint64)      # (number, 3)
        head.combination_root = proof_stream.pull()
        head.indices = BrainfuckStark.sample_indices(self.security_level, proof_stream.verifier_fiat_shamir(), self.fri.domain.length)
        return head

    def _verify_opened_rows(self, proof_stream, head):
        """{row index: canonical limbs of its randomizer, base and extension elements}, every opened row checked against its root (:415-433)"""
        n, rows, unit_distances = self.fri.domain.length, {}, self._layout.unit_distances(self.fri.domain.length)
        for index in head.indices:
            for distance in [0] + unit_distances:
                idx = (index + distance) % n
                element = proof_stream.pull()
                salt, path = proof_stream.pull()
                assert SaltedMerkle.verify(head.base_root, idx, salt, path, element), "salted base tree verify must succeed for base codewords"
                row = [_canonical_limbs(e) for e in element]
                element = proof_stream.pull()
                salt, path = proof_stream.pull()
                assert SaltedMerkle.verify(head.extension_root, idx, salt, path, element), "salted base tree verify must succeed for extension codewords"
                rows[idx] = row + [_canonical_limbs(e) for e in element]
        return rows

    def _combination_terms(self, head, rows, index, shifts):
        """the terms of the non-linear combination at domain point `index` (:435-560), from the opened rows: the randomizer, then every
        term of the layout followed by its shifted copy"""
        P, xscale, layout = air.P, air.xscale, self._layout
        n, challenges, terminals = self.fri.domain.length, head.challenges, head.terminals
        x = self.fri.domain.offset.value * pow(self.fri.domain.omega.value, index, P) % P
        powers = {}                 # x^shift for the few distinct shifts of a proof (151 terms share ~20 degree bounds)

        def with_shifted(value, s):
            f = powers.get(shifts[s])
            if f is None:
                f = powers[shifts[s]] = pow(x, shifts[s], P)
            return [value, xscale(value, f)]
        row = rows[index]
        terms = [row[0]]
        for s in range(layout.num_columns):
            terms += with_shifted(row[1 + s], s)
        # the rows of every table at this point and at the next one: base columns, then its extension columns
        points, next_points = [], []
        for k, table in enumerate(self.tables):
            columns, next_columns = row[1:], rows[(index + table.unit_distance(n)) % n][1:]
            points.append(columns[layout.base[k]] + columns[layout.ext[k]])
            next_points.append(next_columns[layout.base[k]] + next_columns[layout.ext[k]])
        boundary_inverse = pow((x - 1) % P, P - 2, P)
        for k, table in enumerate(self.tables):
            omicron_inverse = pow(table.omicron.value, P - 2, P)
            transition_factor = 0 if table.height == 0 else (x - omicron_inverse) * pow((pow(x, table.height, P) - 1) % P, P - 2, P) % P
            # one over the zerofier of the boundary, the transition and the terminal constraints
            factors = (boundary_inverse, transition_factor, pow((x - omicron_inverse) % P, P - 2, P))
            s = layout.quot[k].start
            for values, factor in zip(table.evaluate_all_constraints(points[k], next_points[k], challenges, terminals), factors):
                for value in values:
                    terms += with_shifted(xscale(value, factor), s)
                    s += 1
        for j, arg in enumerate(self.permutation_arguments):
            terms += with_shifted(xscale(arg.evaluate_difference(points), boundary_inverse), layout.first_argument + j)
        return terms
