"""FRI with one Merkle leaf per folding coset (Fri(..., folding_factor=a, coset_leaves=True)), host side, no GPU: the verifier against
the streams a CPython model of the protocol writes (tests/fri_coset_model.py), the rejections, what the proof saves, the constructor's
and prove()'s argument checks."""
import functools

import pytest

import fri_coset_model as model
import fri_folding_model as per_element

SEED = 0xC05E
OFFSET = 7
T = 4

# every (N, expansion, a) with N = 2^5 .. 2^10, expansion 4 or 16 and at least one fold: F = (log2(N / expansion) - 1) // log2(a) >= 1
CASES = [(N, e, a) for N in (32, 64, 128, 256, 512, 1024) for e in (4, 16) for a in (2, 4, 8)
         if N > e and model.num_folds(N, e, a.bit_length() - 1) >= 1]
TAMPER_CASES = [(32, 4, 4), (64, 4, 8), (256, 4, 2), (512, 4, 4), (1024, 4, 8), (1024, 16, 4)]


@pytest.fixture(scope="session")
def sb():
    from stark_brainfuck_amd import build
    build.build_library()
    import stark_brainfuck_amd
    return stark_brainfuck_amd


@functools.lru_cache(maxsize=None)
def _model(N, expansion, a, extra_degree=0):
    from oracle import ref_oracle as o
    omega = o.primitive_nth_root(N)
    cw = model.codeword_of(o, SEED + N + expansion, N, expansion, OFFSET, omega, extra_degree)
    out = model.prove(o, cw, OFFSET, omega, expansion, T, a)
    out["bytes"] = out["proof_stream"].serialize()
    out["codeword"] = cw
    return out


@functools.lru_cache(maxsize=None)
def _per_element(N, expansion, a):
    from oracle import ref_oracle as o
    out = per_element.prove(o, _model(N, expansion, a)["codeword"], OFFSET, o.primitive_nth_root(N), expansion, T, a)
    out["bytes"] = out["proof_stream"].serialize()
    return out


def _fri(sb, N, expansion, a, **kw):
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    assert BF.generator().value == OFFSET
    kw.setdefault("coset_leaves", True)
    return sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, expansion, T, XF, folding_factor=a, **kw)


def _stream(sb, objects):
    ps = sb.ProofStream()
    ps.objects = list(objects)
    return ps


def _layer_depths(N, expansion, a):
    """log2 q_i for i < F"""
    k = a.bit_length() - 1
    F = model.num_folds(N, expansion, k)
    return [(N >> (k * (i + 1))).bit_length() - 1 for i in range(F)]


def test_the_cases_cover_what_they_should():
    assert {N for N, _, _ in CASES} == {32, 64, 128, 256, 512, 1024} and {e for _, e, _ in CASES} == {4, 16}
    for a in (2, 4, 8):
        folds = {model.num_folds(N, e, a.bit_length() - 1) for N, e, a_ in CASES if a_ == a}
        assert 1 in folds and max(folds) >= 2, (a, folds)       # F = 1: the first layer is the last one; F >= 2: a layer checked against the next
    assert all(case in CASES for case in TAMPER_CASES)
    assert {model.num_folds(N, e, a.bit_length() - 1) == 1 for N, e, a in TAMPER_CASES} == {True, False}


@pytest.mark.parametrize("N,expansion,a", CASES)
def test_model_stream_is_accepted_and_consumed(sb, N, expansion, a):
    ref = _model(N, expansion, a)
    k = a.bit_length() - 1
    F = model.num_folds(N, expansion, k)
    fri = _fri(sb, N, expansion, a)
    assert fri.coset_leaves is True and fri.num_rounds() == F + 1 == ref["rounds"]
    assert [c.shape[1] for c in ref["codewords"]] == [N >> (k * r) for r in range(F + 1)]
    # F roots (rounds 1 .. F), the last codeword, per layer t tuples and t paths
    assert len(ref["proof_stream"].objects) == F + 1 + 2 * F * T
    vs = sb.ProofStream().deserialize(ref["bytes"])
    assert fri.verify(vs, ref["roots"][0]) is True
    assert vs.read_index == len(vs.objects)
    assert fri.verify(_stream(sb, vs.objects), ref["roots"][0]) is True
    # the root the caller hands over is the coset root of C_0, not the per-element one
    assert ref["roots"][0] != _per_element(N, expansion, a)["roots"][0]


@pytest.mark.parametrize("N,expansion,a", CASES)
def test_digest_count_and_proof_size(N, expansion, a):
    ref, old = _model(N, expansion, a), _per_element(N, expansion, a)
    objects = ref["proof_stream"].objects
    assert model.count_digests(objects) == T * sum(_layer_depths(N, expansion, a))
    k = a.bit_length() - 1
    F = model.num_folds(N, expansion, k)
    lengths = [N >> (k * i) for i in range(F + 1)]
    # the per-element protocol: a paths of depth log2 len(C_i) per layer and test, plus one into every next tree but the last
    assert model.count_digests(old["proof_stream"].objects) == \
        T * sum(a * (lengths[i].bit_length() - 1) + ((lengths[i + 1].bit_length() - 1) if i + 1 < F else 0) for i in range(F))
    assert len(ref["bytes"]) < len(old["bytes"]), \
        "coset-leaf stream %d bytes, per-element stream %d bytes (N = %d, expansion %d, a = %d)" % (len(ref["bytes"]), len(old["bytes"]), N, expansion, a)
    assert ref["indices"] != [] and all(0 <= i < N // a for i in ref["indices"])


@pytest.mark.parametrize("N,expansion,a", TAMPER_CASES)
def test_changes_are_rejected(sb, N, expansion, a, capsys):
    ref = _model(N, expansion, a)
    fri = _fri(sb, N, expansion, a)
    XF = sb.ExtensionField.main()
    k = a.bit_length() - 1
    F = ref["rounds"] - 1
    objects = sb.ProofStream().deserialize(ref["bytes"]).objects
    root0 = ref["roots"][0]
    other = XF.from_limbs([1, 2, 3])
    tuples_of = lambda layer: F + 1 + 2 * T * layer          # first of the t tuples of a layer; its paths follow T further on
    assert all(isinstance(objects[tuples_of(i) + s], tuple) and len(objects[tuples_of(i) + s]) == a for i in range(F) for s in range(T))
    assert all(isinstance(objects[tuples_of(i) + T + s], list) for i in range(F) for s in range(T))
    PATH, LINE, LAST = ("merkle authentication path verification fails for the opened coset\n", "colinearity check failure\n",
                        "leafs in last round do not correspond to last codeword\n")

    def verdict(change):
        objs = list(objects)
        change(objs)
        capsys.readouterr()
        return fri.verify(_stream(sb, objs), root0), capsys.readouterr().out

    assert verdict(lambda objs: None) == (True, "")

    # an element of a tuple, every position of the first layer's first tuple: the leaf no longer hashes to the root; when the first
    # layer is also the last, the value it folds to is compared with the last codeword before the path is looked at
    for j in range(a):
        def element(objs, j=j):
            objs[tuples_of(0)] = objs[tuples_of(0)][:j] + (other,) + objs[tuples_of(0)][j + 1:]
        assert verdict(element) == (False, LAST if F == 1 else PATH), j
    if F > 1:
        # the element of a second-layer tuple that the first layer folds to: caught as soon as the tuple arrives
        q1 = N >> (2 * k)
        at = (ref["indices"][0] % (N >> k)) // q1

        def linked(objs):
            objs[tuples_of(1)] = objs[tuples_of(1)][:at] + (other,) + objs[tuples_of(1)][at + 1:]
        assert verdict(linked) == (False, LINE)

    # an element of the last layer's tuple (not the one the layer before checks): the fold no longer lands on the last codeword
    def last_layer(objs):
        i = tuples_of(F - 1) + T - 1
        qF = N >> (k * F)
        skip = (ref["indices"][T - 1] % (qF << k)) // qF if F > 1 else -1
        j = 0 if skip != 0 else 1
        objs[i] = objs[i][:j] + (other,) + objs[i][j + 1:]
    assert verdict(last_layer) == (False, LAST)

    # tuples of a + 1 and a - 1 elements, and something that is no tuple
    for bad in (lambda tup: tup + (other,), lambda tup: tup[:-1], lambda tup: list(tup), lambda tup: tup[:-1] + (b"x",)):
        def shape(objs, bad=bad):
            objs[tuples_of(0) + 1] = bad(objs[tuples_of(0) + 1])
        assert verdict(shape) == (False, LINE)

    # paths: a node changed, one node more, one node less, not a list
    for bad in (lambda p: [bytes(64)] + p[1:], lambda p: p[:-1] + [bytes(64)], lambda p: p + [bytes(64)], lambda p: p[:-1], lambda p: tuple(p),
                lambda p: [7] * len(p)):
        def path(objs, bad=bad):
            objs[tuples_of(0) + T] = bad(list(objs[tuples_of(0) + T]))
        assert verdict(path) == (False, PATH), bad

    # two tuples swapped (tests 0 and 1 of the first layer): each is checked at the other's index
    def swapped(objs):
        i = tuples_of(0)
        objs[i], objs[i + 1] = objs[i + 1], objs[i]
    ok, said = verdict(swapped)
    assert ok is False and said in (PATH, LAST, LINE)

    # a root: every challenge after it changes; the caller's root
    def root(objs):
        objs[0] = bytes(64)
    assert verdict(root)[0] is False
    assert fri.verify(_stream(sb, objects), bytes(64)) is False
    assert fri.verify(_stream(sb, objects), _per_element(N, expansion, a)["roots"][0]) is False

    # the last codeword: an element changed (its root is in the stream), two elements swapped
    def last_element(objs):
        objs[F] = [other] + list(objs[F][1:])
    assert verdict(last_element) == (False, "last codeword is not well formed\n")

    def last_swapped(objs):
        objs[F] = [objs[F][1], objs[F][0]] + list(objs[F][2:])
    assert verdict(last_swapped) == (False, "last codeword is not well formed\n")


@pytest.mark.parametrize("N,expansion,a", TAMPER_CASES)
def test_a_stream_made_in_per_element_mode_is_rejected(sb, N, expansion, a, capsys):
    old, new = _per_element(N, expansion, a), _model(N, expansion, a)
    capsys.readouterr()
    for root in (old["roots"][0], new["roots"][0]):
        assert _fri(sb, N, expansion, a).verify(sb.ProofStream().deserialize(old["bytes"]), root) is False
    assert capsys.readouterr().out == 2 * "colinearity check failure\n"       # (its tuples have a + 1 elements)
    # and the per-element verifier of the same shape accepts it: the two modes differ in nothing but the commitment
    assert _fri(sb, N, expansion, a, coset_leaves=False).verify(sb.ProofStream().deserialize(old["bytes"]), old["roots"][0]) is True


@pytest.mark.parametrize("N,expansion,a", TAMPER_CASES)
def test_last_codeword_of_too_high_a_degree_is_rejected(sb, N, expansion, a, capsys):
    """the degree check of the last codeword is the per-element protocol's: an honest prover on a codeword of degree N / expansion"""
    ref = _model(N, expansion, a, extra_degree=1)
    capsys.readouterr()
    assert _fri(sb, N, expansion, a).verify(sb.ProofStream().deserialize(ref["bytes"]), ref["roots"][0]) is False
    assert capsys.readouterr().out == ""


def test_constructor_and_argument_checks(sb):
    XF = sb.ExtensionField.main()
    BF = XF.modulus.coefficients[0].field
    make = lambda N, expansion, **kw: sb.Fri(BF.generator(), BF.primitive_nth_root(N), N, expansion, T, XF, **kw)
    assert make(1024, 4).coset_leaves is False and make(1024, 4, folding_factor=8).coset_leaves is False
    for a in (2, 4, 8):
        fri = make(1024, 4, folding_factor=a, coset_leaves=True)
        assert fri.coset_leaves is True and fri.folding_factor == a
        assert fri.num_rounds() == make(1024, 4, folding_factor=a).num_rounds()
    for bad in (1, 0, None, "yes", 2):
        with pytest.raises(AssertionError):
            make(1024, 4, coset_leaves=bad)
    # fewer than one fold: folding by 2 tolerates a single round in the per-element mode, not here
    assert make(8, 4).num_rounds() == 1
    for N, expansion, a in [(8, 4, 2), (32, 16, 4), (64, 16, 8)]:
        with pytest.raises(AssertionError):
            make(N, expansion, folding_factor=a, coset_leaves=True)
    with pytest.raises(AssertionError):
        make(1024, 4, folding_factor=3, coset_leaves=True)
    # prove(): known_leafs has no meaning in this mode; round0_tree must be a CosetMerkle of this shape (checked before any GPU work)
    assert issubclass(sb.CosetMerkle, sb.Merkle) and sb.CosetMerkle.verify is sb.Merkle.verify
    codeword = [XF.from_limbs([i + 1, 2, 3]) for i in range(64)]
    fri = make(64, 4, folding_factor=4, coset_leaves=True)
    with pytest.raises(AssertionError, match="known_leafs"):
        fri.prove(codeword, sb.ProofStream(), known_leafs={0: codeword[0]})

    class NotATree:
        coset_size, num_leafs = 4, 16
    with pytest.raises(AssertionError, match="round0_tree"):
        fri.prove(codeword, sb.ProofStream(), round0_tree=NotATree())
    shaped = lambda a, leaves: type("Shaped", (sb.CosetMerkle,), {"__init__": lambda self: None, "coset_size": a, "num_leafs": leaves})()
    for a, leaves in ((2, 32), (8, 8), (4, 8), (4, 32)):
        with pytest.raises(AssertionError, match="round0_tree"):
            fri.prove(codeword, sb.ProofStream(), round0_tree=shaped(a, leaves))
    with pytest.raises(AssertionError, match="CosetMerkle"):
        make(64, 4, folding_factor=4).prove(codeword, sb.ProofStream(), round0_tree=shaped(4, 16))
    for bad in (3, 16, 1):
        with pytest.raises(AssertionError):
            sb.CosetMerkle(codeword, bad)
