"""The scan primitive of include/bfstark.h (bfs_xfe_scan, bfs_xfe_scan_device) restated on Python integers, row after row.  Nothing here
calls the package: the arithmetic of F_p[X] / (X^3 - X + 1), p = 2^64 - 2^32 + 1, is written out below.

Over rows i = 0 .. n - 1, with base-field columns x1, x2, x3 (None = absent), an optional row mask (None = every row), constants
c0 .. c3 and an initial state (extension elements, triples of limbs, reduced mod p on entry as the header says):

    kind 0 (running product):      state <- state * (c0 - c1 x1[(i + shift1) mod n] - c2 x2[i] - c3 x3[i])
    kind 1 (running evaluation):   state <- state * c0 + c1 x1[(i + shift1) mod n] + c2 x2[i] + c3 x3[i]

on the rows the mask lets in; the state is recorded for every row before or after that row's update; the last state is the terminal.
`shift1` applies to the first column only, cyclically, and is taken mod n."""
P = (1 << 64) - (1 << 32) + 1
X0, X1 = (0, 0, 0), (1, 0, 0)


def xadd(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P, (a[2] + b[2]) % P)


def xsub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P, (a[2] - b[2]) % P)


def xscale(a, s):
    return (a[0] * s % P, a[1] * s % P, a[2] * s % P)


def xmul(a, b):
    """schoolbook product, then X^3 = X - 1 and X^4 = X^2 - X"""
    a0, a1, a2 = a
    b0, b1, b2 = b
    d3, d4 = a1 * b2 + a2 * b1, a2 * b2
    return ((a0 * b0 - d3) % P, (a0 * b1 + a1 * b0 + d3 - d4) % P, (a0 * b2 + a1 * b1 + a2 * b0 + d4) % P)


def scan(kind, columns, mask, n, constants, initial, record_before, shift1=0):
    """-> (the three limb planes of the recorded states, three lists of n integers; the terminal triple).  columns: up to three
    sequences of n integers below p, or None; mask: n truth values or None; constants: up to four triples (missing ones are zero)."""
    assert kind in (0, 1)
    columns = list(columns) + [None] * (3 - len(columns))
    c = [tuple(v % P for v in t) for t in constants] + [X0] * (4 - len(constants))
    x1, x2, x3 = columns
    shift = shift1 % n if n and x1 is not None else 0
    state = tuple(v % P for v in initial)
    planes = ([0] * n, [0] * n, [0] * n)
    for i in range(n):
        if record_before:
            planes[0][i], planes[1][i], planes[2][i] = state
        if mask is None or mask[i]:
            lin = X0
            if x1 is not None:
                lin = xadd(lin, xscale(c[1], x1[(i + shift) % n]))
            if x2 is not None:
                lin = xadd(lin, xscale(c[2], x2[i]))
            if x3 is not None:
                lin = xadd(lin, xscale(c[3], x3[i]))
            state = xmul(state, xsub(c[0], lin)) if kind == 0 else xadd(xmul(state, c[0]), lin)
        if not record_before:
            planes[0][i], planes[1][i], planes[2][i] = state
    return planes, state
