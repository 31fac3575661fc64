"""lde_tables without blinding and PolynomialCommitment without hiding on one small case each, as SHA-256 digests of what they leave:
the buffers of lde_tables(..., keep_coefficients=True) over the padded tables of the `,.,.` fixture on seeded randomness, base and
extension columns, and the proof stream of commit + open over two fixed polynomials.  tests/golden/deep_plain_paths.json holds the digests
of the commit BEFORE these functions learnt `blinding` and `hiding`; tests/test_gpu_deep_zk.py compares.

    python tests/deep_plain_paths.py [--root DIR] --write FILE        (needs the GPU; --root: the checkout whose package is measured)
"""
import hashlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
P = (1 << 64) - (1 << 32) + 1
NAME, TAG = "two_io", b"deep-plain-paths"


def _digest(buffer, words):
    return hashlib.sha256(np.ascontiguousarray(buffer.to_numpy()[:words]).tobytes()).hexdigest()


def _words(count, seed):
    with np.errstate(over="ignore"):
        return ((np.arange(1, count + 1, dtype=np.uint64) + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)) % np.uint64(P)


def compute():
    """-> the dict of digests, from whatever stark_brainfuck_amd and tools are importable"""
    from stark_brainfuck_amd import randomness
    from stark_brainfuck_amd.arrays import BaseArray, XArray
    from stark_brainfuck_amd.device import synchronize
    from stark_brainfuck_amd.ip import ProofStream
    from stark_brainfuck_amd.pcs import PolynomialCommitment
    from stark_brainfuck_amd.table import extend_tables_device, lde_tables, prepare_extension, sample_ext
    from tools import deep_stark_time as deep
    from tools import stark_fri_modes as modes
    out = {}
    stark = deep.make_stark(NAME)
    processor, memory, instruction, given, printed = deep.claim(NAME)[4]
    stark._pad_tables(SimpleNamespace(matrices=(processor, instruction, memory, given, printed), proof_stream=None))
    domain, n = stark.fri.domain, stark.fri.domain.length
    stream = modes.Stream(TAG)
    with randomness.override(stream):
        codewords, coefficients, stride = lde_tables(stark.tables, domain, keep_coefficients=True)
        synchronize()
        out["base"] = {"stride": stride, "codewords": _digest(codewords, 16 * n), "coefficients": _digest(coefficients, 16 * stride)}
        challenges = tuple((7 + i, 11 + i, 13 + i) for i in range(11))
        initials = [sample_ext(stream(24)) for _ in stark.permutation_arguments]
        extend_tables_device(stark.tables, challenges, initials, prepared=prepare_extension(stark.tables))
        codewords, coefficients, stride = lde_tables(stark.tables, domain, extension=True, keep_coefficients=True)
        synchronize()
        out["extension"] = {"stride": stride, "codewords": _digest(codewords, 27 * n), "coefficients": _digest(coefficients, 27 * stride)}
    out["bytes_drawn"] = stream.pos
    pc = PolynomialCommitment(deep.make_stark("plus1").fri)          # 2^8 points, 64 coefficients
    polys = [XArray.from_numpy(_words(3 * 64, 1).reshape(3, 64)), BaseArray.from_numpy(_words(40, 2))]
    proof_stream = ProofStream()
    committed = pc.commit(polys, proof_stream)
    z = pc.xfield.sample(proof_stream.prover_fiat_shamir())
    pc.open(committed, [z], proof_stream)
    out["commit_open"] = {"root": committed.root().hex(), "stream": hashlib.sha256(proof_stream.serialize()).hexdigest()}
    return out


if __name__ == "__main__":
    root = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else os.path.dirname(HERE)
    sys.path.insert(0, os.path.abspath(root))
    with open(sys.argv[sys.argv.index("--write") + 1], "w") as fh:
        json.dump({"made_by": "tests/deep_plain_paths.py --root <a checkout of the parent commit> --write", "digests": compute()}, fh, indent=1, sort_keys=True)
        fh.write("\n")
