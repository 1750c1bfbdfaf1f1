"""The rule of gsim_rowhash_*, gsim_row_hash and gsim_duplicates (include/gpusim_hip.h) restated in numpy: the oracle of
tests/test_rowhash_host.py, tests/test_gpu_rowhash.py and tests/test_gpu_rowhash_large.py.  Nothing here calls the library.

  groups(rows, base)             first, size and the counts, from np.unique over whole rows
  find(rows, queries, base)      row, size per query (ROW_NONE, 0: no identical row)
  row_hash(rows)                 the header's 64-bit hash, vectorised uint32 arithmetic
  slots(n), first_slot(hash, n)  the header's slot rule
  colliding_rows(...)            distinct rows whose first slot is a given one, by rejection sampling"""
import numpy as np

ROW_NONE = 0xFFFFFFFF
MIN_SLOTS = 1024
GOLD = 0x9E3779B9


def _as_rows(rows):
    r = np.ascontiguousarray(rows, dtype=np.uint32)
    assert r.ndim == 2
    return r


def groups(rows, base=0):
    """first[i] (the lowest row identical to row i, + base), size[i], and a dict of the counts stats must show"""
    r = _as_rows(rows)
    n = len(r)
    if n == 0:
        z = np.zeros(0, np.uint32)
        return z, z.copy(), dict(rows=0, groups=0, repeated_groups=0, largest_group=0, slots=0)
    _, inverse, counts = np.unique(r, axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    lowest = np.full(len(counts), n, np.int64)
    np.minimum.at(lowest, inverse, np.arange(n))
    first = (lowest[inverse] + base).astype(np.uint32)
    size = counts[inverse].astype(np.uint32)
    return first, size, dict(rows=n, groups=len(counts), repeated_groups=int((counts >= 2).sum()), largest_group=int(counts.max()), slots=slots(n))


def find(rows, queries, base=0):
    """row[q], size[q] of the table `rows` for every query"""
    r, q = _as_rows(rows), _as_rows(queries)
    first, size, _ = groups(r, base)
    where = {}
    for i in range(len(r) - 1, -1, -1):
        where[r[i].tobytes()] = i
    at = np.array([where.get(x.tobytes(), -1) for x in q], np.int64)
    row = np.where(at >= 0, first[np.maximum(at, 0)] if len(r) else 0, ROW_NONE).astype(np.uint32)
    sz = np.where(at >= 0, size[np.maximum(at, 0)] if len(r) else 0, 0).astype(np.uint32)
    return row, sz


def _m1(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x85EBCA6B)
    x = x ^ (x >> np.uint32(13))
    x = x * np.uint32(0xC2B2AE35)
    return x ^ (x >> np.uint32(16))


def _m2(x):
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x2C1B3C6D)
    x = x ^ (x >> np.uint32(12))
    x = x * np.uint32(0x297A2D39)
    return x ^ (x >> np.uint32(15))


def row_hash(rows):
    """The header's hash of every row, uint64 [n]"""
    w = _as_rows(rows)
    with np.errstate(over="ignore"):
        k = ((np.arange(w.shape[1], dtype=np.uint64) + 1) * GOLD).astype(np.uint32)[None, :]  # (the low 32 bits: mod 2^32)
        a = (w ^ k) * np.uint32(0x85EBCA6B)
        a = a ^ (a >> np.uint32(15))
        b = (((w << np.uint32(16)) | (w >> np.uint32(16))) + k) * np.uint32(0xC2B2AE35)
        b = b ^ (b >> np.uint32(13))
        A = a.sum(axis=1, dtype=np.uint32)
        B = b.sum(axis=1, dtype=np.uint32)
        lo = _m1(A ^ _m2(B))
        hi = _m2(B ^ lo)
    return (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)


def slots(n):
    if n == 0:
        return 0
    s = MIN_SLOTS
    while s < 2 * n:
        s *= 2
    return s


def first_slot(h, n):
    return np.asarray(h, np.uint64) & np.uint64(slots(n) - 1)


def colliding_rows(rng, n, W, slot, count):
    """`count` distinct rows of W words whose first slot in a table of n rows is `slot`, by rejection sampling"""
    out, seen = [], set()
    while len(out) < count:
        cand = rng.integers(0, 2 ** 32, (8192, W), dtype=np.uint32) & rng.integers(0, 2 ** 32, (8192, W), dtype=np.uint32)
        for x in cand[first_slot(row_hash(cand), n) == np.uint64(slot)]:
            if x.tobytes() not in seen and len(out) < count:
                seen.add(x.tobytes())
                out.append(x)
    return np.array(out, np.uint32).reshape(count, W)
