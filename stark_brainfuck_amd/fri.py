"""FRI low-degree test, prover on the GPU -- mirror of the reference's `fri.py` (/root/reference/code/fri.py:13-319).

    Fri(offset, omega, initial_domain_length, expansion_factor, num_colinearity_tests, xfield, folding_factor=2, coset_leaves=False,
        grinding_bits=0)
      .domain   Fri.Domain: offset, omega, length, __call__, list, evaluate, xevaluate, interpolate, xinterpolate
      .num_rounds()  .sample_indices(...)  .commit(...)  .query(...)  .query_last(...)  .prove(...)  .verify(...)
    grind(seed, bits, first_nonce=0, count=None)  check_grinding(seed, nonce, bits)

`prove` / `commit` run the whole round loop natively (csrc/fri.hip): Merkle trees, folding and openings on the GPU,
Fiat-Shamir on the host in C++.  `codeword` may be a Python list of ExtensionFieldElement (as in the reference) or an
XArray already in HBM.  `verify` is the verifier: host-side, as in the reference.

`folding_factor` a = 2^k in (2, 4, 8) is how much shorter each round's codeword is than the one before.  2 is the reference's protocol,
byte for byte.  A round of folding by 4 (8) with challenge alpha is two (three) of the reference's split-and-fold steps with the
challenges alpha, alpha^2 (, alpha^4), offset and omega squared between them; the codewords in between are neither kept nor committed
to.  With L = log2(N / expansion_factor) there are F = (L - 1) // k folds and F + 1 codewords; a colinearity test opens, per layer, the
a elements C_i[c + j * q], q = len(C_i) / a, and C_{i+1}[c] as one tuple, then their a (+ 1) authentication paths.

`coset_leaves=True` (with any folding factor) commits to every codeword but the last with ONE MERKLE LEAF PER FOLDING COSET: the tree of
round i < F has q_i = len(C_i) / a leaves, leaf c = blake2b(pickle.dumps((C_i[c], C_i[c + q_i], .., C_i[c + (a - 1) q_i]))) -- `CosetMerkle`
(merkle.py).  A colinearity test then opens, per layer, that tuple of a elements and ONE path of log2 q_i digests; nothing of C_{i+1} is
opened on layer i, because the value the tuple folds to is element number c_i // q_{i+1} of the tuple opened on layer i + 1 (and
last_codeword[c_i] on the last layer).  The caller's root is the coset root of C_0: `CosetMerkle(codeword, a).root()`.  The default,
False, is the per-element protocol above, byte for byte.

`grinding_bits=b`, 1 <= b <= 40 (in any of the modes above), puts a PROOF OF WORK between the commit phase and the queries.  With seed =
the Fiat-Shamir randomness drawn after the last codeword -- the call that yields the index seed when b = 0 -- `prove` pushes the smallest
int n >= 0 for which blake2b(seed + n.to_bytes(8, "little")).digest()[:8], read as a little-endian integer, has its b top bits zero
(`check_grinding`), and samples the indices from the randomness over the stream that holds n.  The search runs on the GPU (`grind`,
csrc/pow.hip); the verifier's check is one hashlib call.  Re-rolling the indices costs a cheating prover 2^b hashes per attempt, so the
conjectured security is t * log2(expansion_factor) + b bits and t can shrink accordingly.  `commit` on its own pushes no nonce: grinding
belongs to `prove`.  The default, 0, pushes nothing: the protocols above, byte for byte.
"""
import ctypes
from hashlib import blake2b

from . import _lib
from .arrays import BaseArray, XArray
from .device import current_stream
from .ip import NativeTranscript, ProofStream
from .merkle import CosetMerkle, Merkle
from .ntt import _base_value, _transform, fast_coset_interpolate
from .univariate import Polynomial, colinear

_u64 = ctypes.c_uint64
MAX_GRINDING_BITS = 40


def check_grinding(seed, nonce, bits):
    """the proof-of-work predicate: blake2b(seed + nonce as 8 little-endian bytes) starts, read as a little-endian 64-bit integer, with
    `bits` zero bits.  hashlib only: the verifier's side."""
    assert len(seed) == 32 and 1 <= bits <= 64 and 0 <= nonce < 1 << 64
    return int.from_bytes(blake2b(bytes(seed) + nonce.to_bytes(8, "little")).digest()[:8], "little") >> (64 - bits) == 0


def grind(seed, bits, first_nonce=0, count=None):
    """the smallest nonce in [first_nonce, first_nonce + count) that `check_grinding` accepts, or None; searched on the GPU
    (bfs_pow_search).  count=None: up to 2^(bits + 6) nonces, where a seed without a hit has probability e^-64."""
    assert len(seed) == 32, "the seed is 32 bytes"
    count = min(1 << (bits + 6), (1 << 64) - first_nonce) if count is None else count
    nonce, found = _u64(), ctypes.c_int()
    _lib.check(_lib.load().bfs_pow_search(bytes(seed), bits, first_nonce, count, ctypes.byref(nonce), ctypes.byref(found), current_stream()))
    return int(nonce.value) if found.value else None


class _Codeword:
    """a round codeword living in HBM that behaves like the reference's list of elements (lazy, identity-stable)."""

    def __init__(self, xarray):
        self.array = xarray
        self._items = None

    def __len__(self):
        return self.array.n

    def _all(self):
        if self._items is None:
            self._items = self.array.to_elements()
        return self._items

    def __getitem__(self, i):
        return self._all()[i]

    def __iter__(self):
        return iter(self._all())


class Fri:
    class Domain:
        def __init__(self, offset, omega, length):
            self.offset = offset
            self.omega = omega
            self.length = length

        def __call__(self, index):
            return (self.omega ^ index) * self.offset

        def list(self):
            out, x = [], self.offset
            for _ in range(self.length):
                out.append(x)
                x = x * self.omega
            return out

        def _evaluate(self, polynomial, as_array):
            coeffs = polynomial.coefficients if isinstance(polynomial, Polynomial) else polynomial
            if isinstance(coeffs, (XArray, BaseArray)):
                src, n_in = coeffs, len(coeffs)
            else:
                assert len(coeffs) <= self.length, "polynomial has more coefficients than the domain has points"
                if not coeffs:
                    return [self.omega.field.zero() for _ in range(self.length)]
                from .extension_field import ExtensionFieldElement
                src = XArray.from_elements(coeffs) if isinstance(coeffs[0], ExtensionFieldElement) else BaseArray.from_elements(coeffs)
                n_in = len(coeffs)
            out = _transform(src, n_in, self.length, _base_value(self.omega), _base_value(self.offset), 1)
            return out if as_array else out.to_elements()

        def evaluate(self, polynomial, as_array=False):
            """coset evaluation of a base-field polynomial (fri.py:26-30)."""
            return self._evaluate(polynomial, as_array)

        def xevaluate(self, polynomial, xfield=None, as_array=False):
            """coset evaluation of an extension-field polynomial (fri.py:32-37): three limb transforms."""
            if xfield is None and isinstance(polynomial, Polynomial):
                assert len(polynomial.coefficients) != 0, "trying to xevaluate zero polynomial with no target field"
            return self._evaluate(polynomial, as_array)

        def interpolate(self, values):
            return fast_coset_interpolate(self.offset, self.omega, values)

        def xinterpolate(self, values):
            return fast_coset_interpolate(self.offset, self.omega, values)

    def __init__(self, offset, omega, initial_domain_length, expansion_factor, num_colinearity_tests, xfield, folding_factor=2, coset_leaves=False,
                 grinding_bits=0):
        assert folding_factor in (2, 4, 8), "folding factor must be 2, 4 or 8"
        assert coset_leaves is True or coset_leaves is False, "coset_leaves must be True or False"
        assert type(grinding_bits) is int and 0 <= grinding_bits <= MAX_GRINDING_BITS, "grinding_bits must be an int from 0 to 40"
        self.coset_leaves = coset_leaves
        self.grinding_bits = grinding_bits
        self._grinding_window = None          # nonces per search step; None: the library's default
        self.domain = Fri.Domain(offset, omega, initial_domain_length)
        self.field = xfield
        self.expansion_factor = expansion_factor
        self.num_colinearity_tests = num_colinearity_tests
        self.folding_factor = folding_factor
        self._log2_folding = folding_factor.bit_length() - 1
        assert self.num_rounds() >= 1, "cannot do FRI with less than one round"
        # (folding by 2 keeps the reference's rule: one round constructs, and prove() fails for want of a second codeword)
        assert folding_factor == 2 or self.num_rounds() >= 2, "cannot do FRI with less than one fold"
        assert not coset_leaves or self.num_rounds() >= 2, "cannot commit to cosets with less than one fold"

    def num_rounds(self):
        """number of codewords: the reference's count of halvings h (fri.py:54-60) when folding by 2, (h - 1) // k + 1 in general"""
        length, rounds = self.domain.length, 0
        while length > self.expansion_factor:
            length //= 2
            rounds += 1
        if self._log2_folding == 1 or rounds == 0:
            return rounds
        return (rounds - 1) // self._log2_folding + 1

    @staticmethod
    def sample_index(byte_array, size):
        return int.from_bytes(bytes(byte_array), "big") % size

    def sample_indices(self, seed, size, reduced_size, number):
        assert number <= reduced_size, \
            f"cannot sample more indices than available in last codeword; requested: {number}, available: {reduced_size}"
        assert number <= 2 * reduced_size, "not enough entropy in indices wrt last codeword"
        indices, reduced, counter = [], set(), 0
        while len(indices) < number:
            index = Fri.sample_index(blake2b(seed + bytes(counter)).digest(), size)
            counter += 1
            if index % reduced_size not in reduced:
                indices.append(index)
                reduced.add(index % reduced_size)
        return indices

    def eval_domain(self):
        return self.domain.list()

    # ------------------------------------------------------------------ prover (GPU)
    def _as_xarray(self, codeword):
        if isinstance(codeword, _Codeword):
            return codeword.array
        return codeword if isinstance(codeword, XArray) else XArray.from_elements(list(codeword))

    def _run_native(self, codeword, proof_stream, with_query, known_leafs=None, round0_tree=None):
        if self.coset_leaves:
            assert not known_leafs, "known_leafs: a Fri that commits to cosets opens whole cosets, the caller cannot hold elements of one"
            assert round0_tree is None or (isinstance(round0_tree, CosetMerkle) and round0_tree.coset_size == self.folding_factor
                                           and round0_tree.num_leafs * self.folding_factor == len(codeword)), \
                "round0_tree must be a CosetMerkle over this codeword with coset_size = the folding factor"
        else:
            assert not isinstance(round0_tree, CosetMerkle), "round0_tree is a CosetMerkle, this Fri commits to single elements"
        lib, stream = _lib.load(), current_stream()
        arr = self._as_xarray(codeword)
        n = len(arr)
        assert n & (n - 1) == 0, "codeword length must be a power of two"
        transcript = proof_stream._native() if hasattr(proof_stream, "_native") else None
        if transcript is None or (transcript.xfield is not None and transcript.xfield is not self.field):
            transcript = NativeTranscript()
            transcript.xfield = self.field
            transcript.scan(proof_stream.objects)
            for o in proof_stream.objects:
                transcript.push(o)
        elif transcript.xfield is None:
            transcript.xfield = self.field
        before = transcript.num_objects()
        session = lib.bfs_fri_session_new()
        try:
            if self._log2_folding != 1:
                _lib.check(lib.bfs_fri_session_set_folding(session, self._log2_folding))
            if self.grinding_bits:
                _lib.check(lib.bfs_fri_session_set_grinding(session, self.grinding_bits, self._grinding_window or 0))
            if self.coset_leaves:
                _lib.check(lib.bfs_fri_session_set_coset_leaves(session, 1))
                if round0_tree is not None and round0_tree._nodes_host is None:
                    _lib.check(lib.bfs_fri_session_round0_coset_tree(session, round0_tree._nodes.ptr, round0_tree.num_leafs, round0_tree.root()))
            elif round0_tree is not None and round0_tree._nodes_host is None and round0_tree.num_leafs == n:
                _lib.check(lib.bfs_fri_session_round0_tree(session, round0_tree._nodes.ptr, round0_tree.root()))
            _lib.check(lib.bfs_fri_commit(session, transcript.handle, arr.ptr, arr.stride, n.bit_length() - 1,
                                          _base_value(self.domain.offset), _base_value(self.domain.omega), self.expansion_factor, stream))
            top = None
            for index, obj in (known_leafs or {}).items():
                # element objects of this codeword that are already in the stream keep their identity (pickle memoises by id)
                # (an int is the handle of an element native code has already put into the transcript)
                _lib.check(lib.bfs_fri_session_alias(session, transcript.handle, 0, index, obj if isinstance(obj, int) else transcript.to_native(obj)))
            if with_query:
                out = (_u64 * self.num_colinearity_tests)()
                _lib.check(lib.bfs_fri_query(session, transcript.handle, self.num_colinearity_tests, out, stream))
                top = [int(x) for x in out]
            if hasattr(proof_stream, "_adopt_lazy"):
                proof_stream._adopt_lazy(transcript, before, transcript.num_objects(), self.field)
            else:
                for i in range(before, transcript.num_objects()):
                    proof_stream.push(transcript.to_python(lib.bfs_ps_object_at(transcript.handle, i), self.field))
            rounds = []
            for r in range(lib.bfs_fri_session_rounds(session)):
                cw, nodes = ctypes.c_void_p(), ctypes.c_void_p()
                length, stride = _u64(), _u64()
                root = ctypes.create_string_buffer(64)
                _lib.check(lib.bfs_fri_session_round(session, r, ctypes.byref(cw), ctypes.byref(length), ctypes.byref(stride), ctypes.byref(nodes), root))
                rounds.append((cw.value, length.value, stride.value, nodes.value, root.raw))
            return top, rounds, session, arr
        except Exception:
            lib.bfs_fri_session_free(session)
            if getattr(proof_stream, "_cached", None) is transcript:
                proof_stream._cached = None          # native code may have appended objects the Python list does not have
            raise

    def commit(self, codeword, proof_stream, round_index=0):
        """fri.py:91-139 -> (codewords, trees); both stay in HBM and are materialised lazily."""
        lib = _lib.load()
        _, rounds, session, arr = self._run_native(codeword, proof_stream, with_query=False)
        keeper = _SessionKeeper(lib, session, arr)
        codewords, trees = [], []
        for r, (cw, length, stride, nodes, _root) in enumerate(rounds):
            view = _Codeword(XArray(_Borrowed(cw, keeper), length, self.field, stride))
            if r == 0 and isinstance(codeword, list):
                view._items = codeword
            if r + 1 == len(rounds):
                view._items = proof_stream.objects[-1]      # fri.py:134 pushes this very list: keep object identity
            codewords.append(view)
            if r + 1 < len(rounds) and self.coset_leaves:
                trees.append(CosetMerkle(view, self.folding_factor, _device_nodes=_Borrowed(nodes, keeper)))
            elif r + 1 < len(rounds):
                trees.append(Merkle(view, _device_nodes=_Borrowed(nodes, keeper)))
        return codewords, trees

    def query(self, current_tree, next_tree, c_indices, proof_stream):
        """fri.py:141-158; folding by a: the a elements c + j * q of the current codeword instead of the two c, c + half"""
        return self._query_layer(current_tree, next_tree.leafs, next_tree, c_indices, proof_stream)

    def query_last(self, current_tree, last_codeword, c_indices, proof_stream):
        """fri.py:160-176: the next codeword is in the stream already, so nothing of it gets a path"""
        return self._query_layer(current_tree, last_codeword, None, c_indices, proof_stream)

    def _query_layer(self, current_tree, next_values, next_tree, c_indices, proof_stream):
        if self.coset_leaves:
            return self._query_cosets(current_tree, c_indices, proof_stream)      # (nothing of the next codeword is opened)
        a, q = self.folding_factor, len(current_tree.leafs) // self.folding_factor
        opened = [[i + j * q for i in c_indices] for j in range(a)]          # (a = 2: a_indices, b_indices)
        for s in range(self.num_colinearity_tests):
            proof_stream.push(tuple(current_tree.leafs[opened[j][s]] for j in range(a)) + (next_values[c_indices[s]],))
        for s in range(self.num_colinearity_tests):
            for j in range(a):
                proof_stream.push(current_tree.open(opened[j][s]))
            if next_tree is not None:
                proof_stream.push(next_tree.open(c_indices[s]))
        return [i for column in opened for i in column]

    def _query_cosets(self, current_tree, c_indices, proof_stream):
        """one layer of the coset protocol: the t opened cosets (tuples of a elements), then their t paths; returns the indices of the
        opened elements, column by column as `query` does"""
        a, q = self.folding_factor, current_tree.num_leafs
        assert isinstance(current_tree, CosetMerkle) and current_tree.coset_size == a, "a Fri that commits to cosets queries CosetMerkle trees"
        for s in range(self.num_colinearity_tests):
            proof_stream.push(current_tree.leafs[c_indices[s]])
        for s in range(self.num_colinearity_tests):
            proof_stream.push(current_tree.open(c_indices[s]))
        return [i + j * q for j in range(a) for i in c_indices]

    def prove(self, codeword, proof_stream, known_leafs=None, round0_tree=None):
        """fri.py:178-199: commit + query in one native call; returns the top-level indices.
        known_leafs: {index: element object} for elements of `codeword` that the caller has already pushed.
        round0_tree: a Merkle tree the caller has already built over `codeword` (round 0 would build the same one)."""
        assert self.domain.length == len(codeword), "initial codeword length does not match length of initial codeword"
        top, _, session, _ = self._run_native(codeword, proof_stream, with_query=True, known_leafs=known_leafs, round0_tree=round0_tree)
        _lib.load().bfs_fri_session_free(session)
        return top

    # ------------------------------------------------------------------ verifier (host, fri.py:201-319)
    def verify(self, proof_stream, root):
        """fri.py:232-319.  Same checks in the same order; the abscissae offset * omega^i and the two polynomial questions -- "has the
        interpolant of the last codeword degree <= d" and "are these three points on a line" -- are answered on integer residues
        (an inverse transform's non-zero pattern, two cross products) instead of through Polynomial objects over element objects:
        the reference's interpolations were 2/3 of this package's 15 ms verifier."""
        from .air import P
        from .merkle import leaf_pickle_source
        if leaf_pickle_source.get() is None and hasattr(proof_stream, "pickle_of"):
            token = leaf_pickle_source.set(proof_stream.pickle_of)      # (a bare Fri.verify on a deserialised stream; see BrainfuckStark.verify)
            try:
                return self.verify(proof_stream, root)
            finally:
                leaf_pickle_source.reset(token)
        omega_v, offset_v = _base_value(self.domain.omega), _base_value(self.domain.offset)
        rounds, t, N = self.num_rounds(), self.num_colinearity_tests, self.domain.length
        roots, alphas = [root], []
        for r in range(rounds):
            if r > 0:
                roots.append(proof_stream.pull())
            alphas.append(self.field.sample(proof_stream.verifier_fiat_shamir()))
        last_codeword = proof_stream.pull()
        if roots[-1] != _host_merkle_root(last_codeword):
            print("last codeword is not well formed")
            return False
        n_last = len(last_codeword)
        degree = (n_last // self.expansion_factor) - 1
        k = self._log2_folding
        last_omega_v = pow(omega_v, 1 << (k * (rounds - 1)), P)
        assert pow(last_omega_v, n_last, P) == 1, "omega does not have right order"
        top = _interpolant_degree(last_omega_v, [tuple(e.limbs()) for e in last_codeword])
        if top > degree:
            return False
        if self.grinding_bits:
            seed = proof_stream.verifier_fiat_shamir()          # over the stream up to the last codeword
            nonce = proof_stream.pull()
            if type(nonce) is not int or not 0 <= nonce < 1 << 64 or not check_grinding(seed, nonce, self.grinding_bits):
                print("proof of work check failure")
                return False
        top_level_indices = self.sample_indices(proof_stream.verifier_fiat_shamir(), N >> k, N >> (k * (rounds - 1)), t)
        return self._verify_layers(proof_stream, roots, alphas, last_codeword, top_level_indices, omega_v, offset_v)

    def _verify_layers(self, proof_stream, roots, alphas, last_codeword, top_level_indices, omega_v, offset_v):
        """the layers of `verify`, one loop for every mode.  With q = len(C_r) / a and c = index mod q, test s opens on layer r
          per element: the tuple (C_r[c], C_r[c + q], .., C_r[c + (a - 1) q], C_{r+1}[c]), then a paths into tree r and -- except on the
            last layer, whose next codeword is in the proof -- one into tree r + 1;
          coset leaves: the tuple of the a values alone, then ONE path of log2 q digests into tree r.  What the tuple folds to is not in
            the stream: it must be element number c_{r-1} // q of the tuple the same test opens on the next layer (`expected`), and
            last_codeword[c] on the last layer -- compared before the paths are pulled; the per-element protocols compare after.
        `_judge` decides a tuple."""
        from .air import P
        rounds, t, N, k, a = self.num_rounds(), self.num_colinearity_tests, self.domain.length, self._log2_folding, self.folding_factor
        coset = self.coset_leaves
        labels = ["the opened coset"] if coset else ["aa", "bb"] if a == 2 else ["opened value %d" % j for j in range(a)]
        expected = None                                   # per test: (position in this layer's tuple, the value the previous layer folded to)
        for r in range(rounds - 1):
            q = N >> (k * (r + 1))
            last_layer = r + 1 == rounds - 1
            c_indices = [i % q for i in top_level_indices]
            opened, nexts = [], []                        # per test: the a elements; what they fold to (coset: a triple, else the opened element)
            for s in range(t):
                judged = self._judge(proof_stream.pull(), alphas[r], offset_v, omega_v, c_indices[s], q, expected[s] if expected else None)
                if judged is None:
                    print("colinearity check failure")
                    return False
                opened.append(judged[0]); nexts.append(judged[1])

            def matches_last_codeword():
                for s in range(t):
                    want = last_codeword[c_indices[s]]
                    if nexts[s] != (tuple(want.limbs()) if coset else want):
                        print("leafs in last round do not correspond to last codeword")
                        return False
                return True
            if coset and last_layer and not matches_last_codeword():
                return False
            for s in range(t):
                if coset:
                    paths = [(roots[r], c_indices[s], opened[s])]
                else:
                    paths = [(roots[r], c_indices[s] + j * q, opened[s][j]) for j in range(a)]
                    if not last_layer:
                        paths.append((roots[r + 1], c_indices[s], nexts[s]))
                for (tree_root, index, leaf), label in zip(paths, labels + ["cc"]):
                    path = proof_stream.pull()
                    well_formed = not coset or (isinstance(path, list) and len(path) == q.bit_length() - 1
                                                and all(isinstance(node, (bytes, bytearray)) for node in path))
                    if not well_formed or not Merkle.verify(tree_root, index, path, leaf):
                        print("merkle authentication path verification fails for " + label)
                        return False
            if not coset and last_layer and not matches_last_codeword():
                return False
            q_next = q >> k
            expected = [(c_indices[s] // q_next, nexts[s]) for s in range(t)] if coset and q_next else None
            for _ in range(k):
                omega_v, offset_v = omega_v * omega_v % P, offset_v * offset_v % P
        return True

    def _judge(self, values, alpha_element, g, w, c, q, expected):
        """one opened tuple of a layer: (the a elements, what they fold to), or None when the tuple fails.  Folding by 2 per element keeps
        the reference's question -- are the three points on a line of degree exactly one (`_on_a_line`; a plain fold comparison would
        accept a constant) -- every other mode compares with `_fold_coset`; `expected`: see _verify_layers."""
        from .air import P
        k, a, alpha = self._log2_folding, self.folding_factor, tuple(alpha_element.limbs())
        if not self.coset_leaves and a == 2:
            ay, by, cy = values
            ax, bx = g * pow(w, c, P) % P, g * pow(w, c + q, P) % P
            on_a_line = _on_a_line(ax, tuple(ay.limbs()), bx, tuple(by.limbs()), alpha, tuple(cy.limbs()))
            if on_a_line is None:          # coinciding abscissae: let the general routine decide (and fail the way the reference's does)
                from .algebra import BaseField, BaseFieldElement
                lift, base = self.field.lift, BaseField.main()
                on_a_line = colinear([(lift(BaseFieldElement(ax, base)), ay), (lift(BaseFieldElement(bx, base)), by), (alpha_element, cy)])
            return ((ay, by), cy) if on_a_line else None
        if not isinstance(values, tuple) or len(values) != (a if self.coset_leaves else a + 1):
            return None
        if self.coset_leaves and not all(hasattr(e, "limbs") for e in values):
            return None
        v = [tuple(e.limbs()) for e in values[:a]]
        if expected is not None and v[expected[0]] != expected[1]:
            return None
        folded = _fold_coset(v, alpha, g, w, c, q, k)
        if self.coset_leaves:
            return values, folded
        return (values[:a], values[a]) if folded == tuple(values[a].limbs()) else None


def _fold_coset(values, alpha, g, w, c, q, k):
    """the a = 2^k values C[c + j q] (integer triples) folded k times: fri.py:127-128 on integer residues, with alpha^(2^step), offset g
    and generator w squared between the steps -- the only copy of the fold arithmetic on the host"""
    from .air import P, xadd, xmul, xscale, xsub
    half_inv = pow(2, P - 2, P)
    v = list(values)
    for _ in range(k):
        h = len(v) // 2
        folded = []
        for m in range(h):
            x_inv = pow(g * pow(w, c + m * q, P) % P, P - 2, P)
            beta = xscale(alpha, half_inv * x_inv % P)
            folded.append(xadd(xscale(xadd(v[m], v[m + h]), half_inv), xmul(beta, xsub(v[m], v[m + h]))))
        v, alpha, g, w = folded, xmul(alpha, alpha), g * g % P, w * w % P
    return v[0]


def _host_merkle_root(leaves):
    """Merkle(leaves).root() (merkle.py:8-44) with hashlib, for the verifier's check of the last codeword -- a few dozen elements.  The
    verifier runs on the host throughout, like the reference's (fri.py:201-319), so verify() needs no GPU; the prover's trees are
    built by the kernels of csrc/merkle.hip and compared with this construction by the tests."""
    from hashlib import blake2b
    from .merkle import leaf_bytes
    n = len(leaves)
    if n == 0 or n & (n - 1):
        return Merkle(leaves).root()            # (never the case for a FRI codeword; the reference's padding rules live in Merkle)
    level = [blake2b(leaf_bytes(e)).digest() for e in leaves]
    while len(level) > 1:
        level = [blake2b(level[2 * i] + level[2 * i + 1]).digest() for i in range(len(level) // 2)]
    return level[0]


def _interpolant_degree(omega, values):
    """degree of the polynomial that takes the extension-field `values` (integer triples) on the coset offset * omega^i, i < n (-1:
    the zero polynomial) -- what `Polynomial.interpolate_domain(...).degree()` answers in fri.py:253-259.  Coefficient j of the
    interpolant is, up to the non-zero factor n * offset^j, sum_i y_i omega^(-i j): the offset does not matter."""
    from .air import P
    n = len(values)
    inverse = pow(omega, P - 2, P)
    for j in range(n - 1, -1, -1):
        step, w, acc = pow(inverse, j, P), 1, (0, 0, 0)
        for y in values:
            acc = ((acc[0] + y[0] * w) % P, (acc[1] + y[1] * w) % P, (acc[2] + y[2] * w) % P)
            w = w * step % P
        if any(acc):
            return j
    return -1


def _on_a_line(ax, ya, bx, yb, cx, yc):
    """univariate.colinear for the verifier's three points (ax, ya), (bx, yb), (cx, yc) -- ax, bx base-field residues, cx and the
    ordinates extension triples: True iff the interpolant has degree exactly 1 (a non-zero slope and equal cross products); None
    when two abscissae coincide (the general routine then decides, and fails, as the reference's does)."""
    from .air import P, xmul, xscale, xsub
    d1, d2, dx = (bx - ax) % P, xsub(cx, (ax, 0, 0)), xsub(cx, (bx, 0, 0))
    if not (d1 and any(d2) and any(dx)):
        return None
    e1 = xsub(yb, ya)
    return bool(any(e1)) and xscale(xsub(yc, ya), d1) == xmul(e1, d2)


class _SessionKeeper:
    """keeps a native FRI session (and the round-0 codeword) alive while views into its HBM block exist."""

    def __init__(self, lib, session, arr):
        self.lib, self.session, self.arr = lib, session, arr

    def __del__(self):
        try:
            self.lib.bfs_fri_session_free(self.session)
        except Exception:
            pass


class _Borrowed:
    """a device pointer owned by someone else, shaped like DeviceBuffer for reads."""

    def __init__(self, ptr, keeper):
        self.ptr, self._keeper = ptr, keeper

    def to_numpy(self, count, offset=0, stream=None):
        import numpy as np
        out = np.empty(count, dtype=np.uint64)
        if count:
            _lib.check(_lib.load().bfs_memcpy_d2h(out.ctypes.data, self.ptr + 8 * offset, count * 8,
                                                  stream if stream is not None else current_stream()))
        return out
