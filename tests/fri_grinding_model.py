"""A CPython model of FRI with proof-of-work grinding (Fri(..., grinding_bits=b)), for tests/test_fri_grinding_host.py and
tests/test_gpu_fri_grinding.py: hashlib, pickle (through `oracle.ProofStreamOracle`) and the two existing models, unchanged.

Protocol.  The commit phase is the mode's own, up to and including the push of the last codeword.  Then
    seed  = prover_fiat_shamir()                                    (32 bytes: the call that yields the index seed without grinding)
    nonce = the smallest n >= 0 with hit(seed, n, b)
    hit(seed, n, b) := int.from_bytes(blake2b(seed + n.to_bytes(8, "little")).digest()[:8], "little") >> (64 - b) == 0
the nonce is pushed as a plain int, and the top-level indices come from prover_fiat_shamir() over the stream that holds it; the queries
are the mode's own.  `prove` gets there without touching the models: it hands them a proof stream whose prover_fiat_shamir, asked right
after the last codeword was pushed (the last object is a list whose items are not bytes -- an authentication path is a list of bytes),
grinds on the value it would have returned, pushes the nonce and answers for the longer stream.  b = 0: the models' own streams.
"""
import hashlib

import fri_coset_model
import fri_folding_model


def hit(seed, nonce, bits):
    return int.from_bytes(hashlib.blake2b(seed + nonce.to_bytes(8, "little")).digest()[:8], "little") >> (64 - bits) == 0


def grind(seed, bits, first=0, count=None):
    """the linear search: the smallest hit in [first, first + count) or None; count=None: no end"""
    n = first
    while count is None or n < first + count:
        if hit(seed, n, bits):
            return n
        n += 1
    return None


def grinding_stream(o, bits, forced_nonce=None):
    """forced_nonce: pushed instead of the smallest hit (a test's forged stream, honest in everything else)"""
    class GrindingStream(o.ProofStreamOracle):
        nonce = seed = None

        def prover_fiat_shamir(self, num_bytes=32):
            value = super().prover_fiat_shamir(num_bytes)
            last = self.objects[-1] if self.objects else None
            if bits and self.nonce is None and isinstance(last, list) and last and not isinstance(last[0], (bytes, bytearray)):
                self.seed, self.nonce = value, grind(value, bits) if forced_nonce is None else forced_nonce
                self.push(self.nonce)
                value = super().prover_fiat_shamir(num_bytes)
            return value
    return GrindingStream()


def prove(o, cw, offset, omega, expansion, t, folding_factor, coset_leaves, bits, proof_stream=None, forced_nonce=None):
    """-> the mode's model's dict, plus "nonce" and "seed" (None when bits = 0).  proof_stream: objects pushed beforehand are taken over"""
    ps = grinding_stream(o, bits, forced_nonce)
    if proof_stream is not None:
        ps.objects = list(proof_stream.objects)
    model = fri_coset_model if coset_leaves else fri_folding_model
    out = model.prove(o, cw, offset, omega, expansion, t, folding_factor, proof_stream=ps)
    out["nonce"], out["seed"] = ps.nonce, ps.seed
    return out
