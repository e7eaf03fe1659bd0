"""NumPy restatement of taco_collate's semantics (include/taco_abi.h), the yardstick of tests/test_gpu_feed.py.

A stream is a dict: pack (1-D array of 4-byte words, float32 or int32), start (int64 [N] or None), rows (int32 [N] or None), width,
rows_out.  Everything is done on the bits (uint32 views), item by item, with Python slices -- no vector tricks the kernel shares."""
import numpy as np


def words(a):
    """Any float32 / int32 array as its uint32 bits."""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4, a.dtype
    return a.view(np.uint32)


def collate_stream(stream, index, N):
    """-> (out [B, rows_out * width] uint32, counts [B] int32, read: boolean mask over the pack of the words that may be read)."""
    pack = words(stream["pack"]).reshape(-1)
    width, rows_out = int(stream["width"]), int(stream["rows_out"])
    start, rows = stream.get("start"), stream.get("rows")
    assert not (start is None and rows is not None)
    B = len(index)
    out = np.zeros((B, rows_out * width), np.uint32)
    counts = np.zeros(B, np.int32)
    read = np.zeros(pack.shape, bool)
    for b, i in enumerate(int(v) for v in index):
        if not 0 <= i < N:
            continue
        c = min(int(rows[i]) if rows is not None else rows_out, rows_out)
        c = max(c, 0)
        s0 = int(start[i]) if start is not None else i * rows_out * width
        out[b, :c * width] = pack[s0:s0 + c * width]
        assert c == 0 or s0 + c * width <= pack.size
        read[s0:s0 + c * width] = True
        counts[b] = c
    return out, counts, read


def collate(streams, index, N):
    return [collate_stream(s, index, N)[:2] for s in streams]
