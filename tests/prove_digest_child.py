"""Child process of tests/test_gpu_commitments_exact.py: proves one program of test_gpu_prover_pointwise.PROGRAMS from its fixed
random stream and prints the SHA-256 of the proof.  The switches of the row-leaf kernels (BFS_ROWS_GENERATED, BFS_ROWS_SPECULATE) are
read once per process, so each setting needs a process of its own.

    python tests/prove_digest_child.py <program name>
"""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (HERE, os.path.dirname(HERE)):
    if path not in sys.path:
        sys.path.insert(0, path)


class _Patch:
    """monkeypatch.setattr for a process that ends after one proof.  setattr is all that _prove asks of its monkeypatch, for
    hello_world (test_gpu_config4._setup) as for the other programs: the three `urandom` names are pointed at the fixed stream."""

    @staticmethod
    def setattr(target, name, value):
        setattr(target, name, value)


def main(name):
    from stark_brainfuck_amd import _lib
    from test_gpu_prover_pointwise import _prove
    lib = _lib.load()
    before = lib.bfs_row_generated_launches()
    stark, proof = _prove(_Patch(), name)
    assert stark.verify(proof) is True
    print("proof %s %d bytes sha256 %s generated_launches %d" % (name, len(proof), hashlib.sha256(proof).hexdigest(),
                                                                 lib.bfs_row_generated_launches() - before))


if __name__ == "__main__":
    main(sys.argv[1])
