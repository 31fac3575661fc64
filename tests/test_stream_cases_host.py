"""The case table of the stream-order tests (tests/stream_cases.py) against include/bfstark.h, and every case's decoy against its real
inputs, on the CPU: a stream-taking entry point is either exercised or excluded for a reason the header itself gives, and a kernel
that read a decoy would be seen in every word the decoy's reference is required to change."""
import os
import re

import numpy as np
import pytest

import stream_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "bfstark.h")) as f:
        return f.read()


def stream_functions(text):
    """every function of the header with a `void* stream` parameter"""
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    found = set()
    for m in re.finditer(r"\b(?:int|void|uint64_t|size_t)\s*\*?\s*(bfs_\w+)\s*\(([^;{}]*?)\)\s*;", code, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            found.add(m.group(1))
    return found


def test_the_parser_finds_the_stream_parameter():
    names = stream_functions(header())
    assert {"bfs_gl_ntt", "bfs_memset", "bfs_stark_finish", "bfs_ptree_build", "bfs_stream_destroy", "bfs_air_combine_rows"} <= names
    assert "bfs_malloc" not in names and "bfs_xfe_scan" not in names and len(names) >= 55


def test_every_stream_taking_entry_point_is_a_case_or_excluded_with_the_headers_words():
    comments = " ".join(re.findall(r"/\*.*?\*/", header(), flags=re.S))           # comment text only: a prototype is no reason
    text = " ".join(re.sub(r"\n\s*\*(?!/)", " ", comments).split())               # ... without the line breaks and their asterisks
    names = stream_functions(header())
    covered = sc.covered()
    assert covered <= names | {"bfs_malloc_async", "bfs_free_async"}, sorted(covered - names)
    assert not covered & set(sc.EXCLUDED), sorted(covered & set(sc.EXCLUDED))
    assert set(sc.INSTRUMENTS) <= names - covered - set(sc.EXCLUDED)
    missing = sorted(names - covered - set(sc.EXCLUDED) - set(sc.INSTRUMENTS))
    assert missing == [], "neither exercised nor excluded: %s" % missing
    for name, reason in list(sc.EXCLUDED.items()) + list(sc.DEVICE_WIDE.items()):
        assert (name in names) == (name in sc.EXCLUDED), name
        assert " ".join(reason.split()) in text, "the reason for leaving %s out is not the header's: %r" % (name, reason)


def test_case_names_and_kinds():
    names = [c.name for c in sc.CASES]
    assert len(set(names)) == len(names)
    kinds = {c.kind for c in sc.CASES}
    assert kinds == {"enqueues", "synchronises"}


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_a_decoy_read_changes_every_compared_word(case):
    fixed = case.fixed()
    assert not set(fixed) & set(case.inputs(0))
    for v in case.variants:
        real, decoy, warm = case.inputs(v), case.inputs(sc.DECOY), case.inputs(sc.WARM)
        assert set(real) == set(decoy) == set(warm)
        for name in real:
            for other in (decoy, warm):
                assert real[name].shape == other[name].shape and real[name].dtype == other[name].dtype, name
                assert not np.array_equal(real[name], other[name]), name
            assert real[name].dtype in (np.dtype(np.uint64), np.dtype(np.uint8))
        want = case.want(real, v)
        assert set(case.outputs) <= set(want), "every device output has a reference"
        for name, words in case.outputs.items():
            assert want[name].size == words, (name, want[name].size, words)
            if name in real:
                assert real[name].dtype == np.uint64 and real[name].size == words
        if not real:
            continue                                  # no device operand: nothing a kernel could read early
        other = case.want(decoy, v)
        differs = False
        for name in want:
            select = case.selected(name, want[name].size)
            sensitive = np.asarray(case.sensitive[name], dtype=np.int64) if name in case.sensitive else select
            assert set(sensitive.tolist()) <= set(select.tolist()), name
            same = np.flatnonzero(want[name][sensitive] == other[name][sensitive])
            assert same.size == 0, "%s: the decoy gives the real input's word at %d of %d places, first at %d" % (
                name, same.size, sensitive.size, sensitive[same[0]])
            differs |= bool((want[name][select] != other[name][select]).any())
        assert differs
    if len(case.variants) == 2:
        a, b = case.want(case.inputs(0), 0), case.want(case.inputs(1), 1)
        assert any((a[name] != b[name]).any() for name in a), "the two calls of the pair must not compute the same"
