"""What tests/test_gpu_stark_fri_modes.py and tests/test_stark_fri_modes_host.py share: a proof read with CPython's pickle into the oracle's
look-alike classes (oracle/ref_oracle.py registers them under the reference's module names) and moved onto the oracle's own field objects, so
that objects made by `oracle.make_xfe` and by the FRI models can stand next to the proof's own in one stream.  No test lives here."""
import pickle


def load(o, proof):
    """the proof's list of objects.  Every extension element of a proof points at ONE ExtensionField instance and every coefficient at the
    BaseField instance inside its modulus; pickle writes each once and refers back to it, so a stream that mixed the proof's instances with
    the oracle's would be a different byte string (and draw different Fiat-Shamir randomness).  Here the proof's elements are pointed at
    the oracle's instances instead: the same graph, the same bytes -- asserted -- on the objects the models build on."""
    objs = pickle.loads(proof)
    probe = o.make_xfe([1, 1, 1])
    xfield, internal = probe.field, probe.polynomial.coefficients[0].field
    seen, stack, theirs = set(), list(objs), None
    while stack:
        x = stack.pop()
        if id(x) in seen:
            continue
        seen.add(id(x))
        if isinstance(x, (list, tuple)):
            stack.extend(x)
        elif hasattr(x, "polynomial"):
            if theirs is None:
                theirs = (x.field, x.field.modulus.coefficients[0].field)
            assert x.field is theirs[0] or x.field is xfield
            x.field = xfield
            stack.extend(x.polynomial.coefficients)
        elif hasattr(x, "value") and theirs is not None and x.field is theirs[1]:
            x.field = internal
    assert o.dumps(objs) == proof
    return objs


def by_value(o, obj):
    """an object of a stream as plain values: elements as limb triples, digests as bytes, ints as ints"""
    if isinstance(obj, (bytes, bytearray)):
        return bytes(obj)
    if type(obj) is int:
        return obj
    if isinstance(obj, (list, tuple)):
        return (type(obj).__name__, [by_value(o, x) for x in obj])
    if hasattr(obj, "polynomial"):
        return ("xfe", tuple(int(v) for v in o.xfe_limbs(obj)))
    if hasattr(obj, "value"):
        return ("bfe", int(obj.value))
    raise AssertionError("unexpected object in a proof stream: %r" % (obj,))
