"""Builders shared by tests/test_gpu_buffer_contracts.py and the stream-order cases (tests/stream_cases.py): strided batches and
Table.pad restated on Python integers."""
import numpy as np

P = (1 << 64) - (1 << 32) + 1
PAD_WIDTH = [7, 3, 4, 1, 1]
PAD_MASKS = [3, 2, 1, 0, 0]


def strided(rows, stride, fill):
    """rows of a (k, n) array laid out `stride` apart in one flat array whose gaps hold `fill`"""
    rows = np.asarray(rows, dtype=np.uint64)
    flat = np.ascontiguousarray(fill[:rows.shape[0] * stride], dtype=np.uint64).copy()
    assert flat.size == rows.shape[0] * stride
    for k, row in enumerate(rows):
        flat[k * stride:k * stride + row.size] = row
    return flat


def padded(kind, rows, width, height):
    """Table.pad restated as in test_trace_padding_on_the_device (processor_table.py:24-35, instruction_table.py:19-25,
    memory_table.py:40-44, io_table.py:17-21): the padded columns and the scan masks of the table's extension"""
    k = rows.shape[0]
    vals = [[int(v) % P for v in r[:width]] for r in rows]
    out = [[0] * height for _ in range(width)]
    for r in range(k):
        for c in range(width):
            out[c][r] = vals[r][c]
    last = vals[-1] if k else [0] * width
    for r in range(k, height):
        j = r - k + 1
        if kind == 0:
            out[0][r] = (last[0] + j) % P
            for c in (1, 4, 5, 6):
                out[c][r] = last[c]
        elif kind == 1:
            out[0][r] = last[0]
        elif kind == 2:
            out[0][r], out[1][r], out[2][r], out[3][r] = (last[0] + j) % P, last[1], last[2], 1
    masks = []
    if kind == 0:
        masks = [[int(v != 0) for v in out[2]], [int(v == ord(",")) for v in out[2]], [int(v == ord(".")) for v in out[2]]]
    elif kind == 1:
        same = [r > 0 and out[0][r] == out[0][r - 1] for r in range(height)]
        masks = [[int(out[1][r] != 0 and same[r]) for r in range(height)], [int(not s) for s in same]]
    elif kind == 2:
        masks = [[int(v == 0) for v in out[3]]]
    return out, masks
