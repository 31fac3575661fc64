"""Operands and configurations for the scan primitive (bfs_xfe_scan / bfs_xfe_scan_device / bfs_xfe_scan_device_many), shared by
tests/test_extend_host.py (host primitive, the sizes that are cheap on a CPU) and tests/test_gpu_extend.py.  Nothing here calls the
package; the expected values come from scan_model.scan.

Sizes sit on every edge of the device's partition (scan_fill in csrc/scan.hip: at most 256 workgroups of 256 threads, each thread
taking `items` consecutive rows): 1, 255, 256, 257; 65 535 / 65 536 / 65 537, where items goes from 1 to 2, the last workgroup holds
one row and most of its threads start past n; 131 072 / 131 073, where items goes from 2 to 3."""
import itertools
import random

from field_states import PALETTE
from scan_model import P, X0, xadd, xscale

SMALL_SIZES = (1, 255, 256, 257)
LARGE_SIZES = (65535, 65536, 65537, 131072, 131073)
PRESENT = tuple(itertools.product((False, True), repeat=3))          # which of x1, x2, x3 exist: every set, the empty one included
MASKS = ("absent", "none", "first", "last", "blocks")
_CACHE = {}


def operands(n, mode):
    """-> (three columns of n residues, constants c0..c3, initial).  "palette": palette values cycling through columns, constants and
    initial; "random": random residues, the first column all distinct (i -> i * odd + 12345 mod p is injective below p) so that a
    wrong `shift1` cannot hide"""
    key = (n, mode)
    if key not in _CACHE:
        rng = random.Random((n << 1) | (mode == "random"))
        if mode == "palette":
            cols = [[PALETTE[(i + 5 * c) % len(PALETTE)] for i in range(n)] for c in range(3)]
            constants = [tuple(PALETTE[(7 * j + 3 * l + 1) % len(PALETTE)] for l in range(3)) for j in range(4)]
            initial = (PALETTE[14], PALETTE[3], PALETTE[8])
        else:
            cols = [[(i * 0x9E3779B97F4A7C15 + 12345) % P for i in range(n)]] + [[rng.randrange(P) for _ in range(n)] for _ in range(2)]
            constants = [tuple(rng.randrange(P) for _ in range(3)) for _ in range(4)]
            initial = tuple(rng.randrange(P) for _ in range(3))
        _CACHE[key] = (cols, constants, initial)
    return _CACHE[key]


def mask(n, which):
    """"absent": no mask; "none": all zero (the output is the initial value everywhere); "first" / "last": one row; "blocks": zero
    across whole workgroups -- only the last 100 rows take part (row 0 too when n >= 512), so every workgroup but the last (and the
    first) composes identities only; "most": three rows of four"""
    if which == "absent":
        return None
    if which == "none":
        return [0] * n
    if which == "first":
        return [1] + [0] * (n - 1)
    if which == "last":
        return [0] * (n - 1) + [1]
    if which == "blocks":
        m = [0] * n
        for i in range(max(n - 100, 0), n):
            m[i] = 1
        if n >= 512:
            m[0] = 1
        return m
    rng = random.Random(n)
    return [int(rng.randrange(4) != 0) for _ in range(n)]


def config(n, mode, kind, present, mask_name, before, shift1=0, zero_row=None, zero_c0=False):
    """one scan as the arguments of scan_model.scan plus a label.  zero_row: c0 is solved so that the factor of that row of a product
    is exactly zero (every later state is 0); zero_c0: c0 = 0, the evaluation forgets its state on every row"""
    cols, constants, initial = operands(n, mode)
    cols = [c if p else None for c, p in zip(cols, present)]
    constants = list(constants)
    if zero_c0:
        constants[0] = X0
    if zero_row is not None:
        assert kind == 0
        lin = X0
        for j, c in enumerate(cols):
            if c is not None:
                lin = xadd(lin, xscale(constants[j + 1], c[(zero_row + shift1) % n if j == 0 else zero_row]))
        constants[0] = lin
    return {"label": (n, mode, kind, present, mask_name, before, shift1, zero_row, zero_c0), "kind": kind, "n": n, "mode": mode,
            "columns": cols, "present": present, "mask_name": mask_name, "mask": mask(n, mask_name), "constants": constants,
            "initial": initial, "before": before, "shift1": shift1, "zero_row": zero_row}


def small_configs(n):
    """every kind x set of present columns x mask x recording mode, the operand sets alternating so that each meets every (kind, set of
    columns); every shift on the distinct first column; c0 = 0; planted zero factors in the middle and at the edges of a workgroup"""
    out = []
    for k, (kind, present, mask_name, before) in enumerate(itertools.product((0, 1), PRESENT, MASKS, (True, False))):
        out.append(config(n, ("palette", "random")[(k + (k // 10)) % 2], kind, present, mask_name, before))
    for shift1 in (0, 1, n - 1, n, n + 1):
        out.append(config(n, "random", 1, (True, False, False), "most", True, shift1))
        out.append(config(n, "random", 0, (True, True, True), "absent", False, shift1))
    for mode in ("palette", "random"):
        out.append(config(n, mode, 1, (True, True, True), "most", False, zero_c0=True))
        out.append(config(n, mode, 1, (False, False, False), "absent", True, zero_c0=True))
    for zero_row in sorted({0, n // 2, 100 % n, 255 % n, n - 1}):
        out.append(config(n, "random", 0, (True, True, True), "absent", zero_row % 2 == 0, zero_row=zero_row))
        out.append(config(n, "palette", 0, (True, False, True), "absent", zero_row % 2 == 1, shift1=1, zero_row=zero_row))
    return out


def large_configs(n):
    """a handful per size (the model takes about a second for 131 073 rows)"""
    k = LARGE_SIZES.index(n)
    shift1 = (1, n - 1, n + 1, n, 1)[k]
    out = [config(n, "random", 0, (True, True, True), "most", True),
           config(n, "palette", 1, (True, False, False), "absent", False, shift1),
           config(n, "random", 1, (True, True, True), "last", True, zero_c0=(k % 2 == 1)) if k % 2 else
           config(n, "palette", 0, (True, True, False), "blocks", False, shift1)]
    if n == 65537:      # two rows per thread, 512 per workgroup: the middle of a workgroup, the last row of one and the first of the next
        out += [config(n, "random", 0, (True, False, False), "absent", z % 2 == 0, zero_row=z) for z in (300, 511, 512)]
    return out


def many_configs():
    """64 scans for one call of bfs_xfe_scan_device_many: kinds, sizes 1 .. 1000 and two large ones (so that the launch is as wide as
    the largest scan and most scans leave most of it idle), masks, shifts and recording modes mixed"""
    rng = random.Random(64)
    sizes = [1, 2, 255, 256, 257, 511, 512, 513, 1000] + [rng.randrange(1, 1001) for _ in range(53)]
    out = []
    for k, n in enumerate(sizes):
        kind = k % 2
        present = PRESENT[(k * 3 + 1) % 8]
        zero_row = n // 2 if kind == 0 and k % 8 == 2 else None           # (no mask there: the row has to take part)
        out.append(config(n, ("palette", "random")[(k // 2) % 2], kind, present, "absent" if zero_row is not None else (MASKS + ("most",))[k % 6],
                          (k // 3) % 2 == 0, shift1=(0, 1, n - 1, n, n + 1)[k % 5] if present[0] else 0,
                          zero_row=zero_row, zero_c0=kind == 1 and k % 8 == 5))
    out.insert(7, config(65537, "random", 1, (True, True, False), "most", False, 1))
    out.insert(40, config(131073, "palette", 0, (True, True, True), "blocks", True))
    assert len(out) == 64
    return out
