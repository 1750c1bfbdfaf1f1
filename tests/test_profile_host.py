"""CPU checks of the column-count calls: the four symbols exist and the stats struct matches the header; gsim_isim against brute-force
pair sums in Python integers, bit for bit as doubles; its 128-bit path at n = 2^32 - 1 and 4096 bits; gsim_isim_complement against
gsim_isim recomputed without each row; every GSIM_ERR_INVALID of the two host functions; gsim_db_bit_counts and gsim_db_overlap_sums
on a table that is not on a GPU: an argument error first, a state error otherwise (never a host computation).
Not checked: GSIM_ERR_INVALID of the two device calls for a table of 2^32 rows or more."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpusimilarity_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, OK = -1, -5, 0
TAN, RR, SM = capi.ISIM_TANIMOTO, capi.ISIM_RUSSELL_RAO, capi.ISIM_SIMPLE_MATCHING
NEW = ["gsim_db_bit_counts", "gsim_db_overlap_sums", "gsim_isim", "gsim_isim_complement"]
U64P = C.POINTER(C.c_uint64)


def message():
    return capi.load().gsim_last_error().decode()


def test_the_symbols_exist_and_the_struct_matches_the_header():
    L = capi.load()
    for name in NEW:
        assert hasattr(L, name) and name in capi.EXPORTS, name
    assert capi.Table.bit_counts and capi.Table.overlap_sums and capi.isim and capi.isim_complement
    text = open(os.path.join(ROOT, "include", "gpusim_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} gsim_profile_stats;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [tuple(d.split()) for d in body.split(";") if d.strip()]
    scalar = {"uint64_t": C.c_uint64, "double": C.c_double}
    assert [(n, scalar[t]) for t, n in fields] == list(capi.GsimProfileStats._fields_)
    assert C.sizeof(capi.GsimProfileStats) == 8 * 7
    for name, value in (("GSIM_ISIM_TANIMOTO", TAN), ("GSIM_ISIM_RUSSELL_RAO", RR), ("GSIM_ISIM_SIMPLE_MATCHING", SM)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
    for name, value in (("STREAMED", capi.PROFILE_STREAMED), ("GATHERED", capi.PROFILE_GATHERED), ("MATRIX", capi.PROFILE_MATRIX),
                        ("VALU", capi.PROFILE_VALU)):
        assert re.search(r"#define\s+GSIM_PROFILE_%s\s+%du\b" % (name, value), text), name
    assert "not the mean of the pairwise Tanimoto scores" in text


def unpack(rows):
    return np.unpackbits(np.ascontiguousarray(rows).view(np.uint8), bitorder="little").reshape(len(rows), -1)


def index_of(a, d, dis, index):
    """the rule on Python integers: one correctly rounded conversion each, one double divide"""
    num = a + d if index == SM else a
    den = a + dis if index == TAN else a + d + dis
    return 0.0 if den == 0 else float(num) / float(den)


def brute(B, index):
    """pair sums over all i < j from the n x n products of the unpacked bits"""
    n, F = B.shape
    B = B.astype(np.int64)
    ones = B @ B.T            # |x_i AND x_j|
    zeros = (1 - B) @ (1 - B).T
    iu = np.triu_indices(n, 1)
    a = int(ones[iu].sum())
    d = int(zeros[iu].sum())
    dis = len(iu[0]) * F - a - d
    return index_of(a, d, dis, index)


def from_counts(counts, n, index):
    c = [int(x) for x in counts]
    return index_of(sum(x * (x - 1) // 2 for x in c), sum((n - x) * (n - x - 1) // 2 for x in c), sum(x * (n - x) for x in c), index)


def random_rows(rng, n, bits, density):
    B = (rng.random((n, bits)) < density).astype(np.uint8)
    return np.packbits(B, axis=1, bitorder="little").view(np.uint32).reshape(n, bits // 32)


def same_double(x, y):
    return np.float64(x).view(np.uint64) == np.float64(y).view(np.uint64)


@pytest.mark.parametrize("bits", [64, 1024])
@pytest.mark.parametrize("n", [2, 3, 50])
def test_isim_equals_the_brute_force_ratio_of_pair_sums(n, bits):
    rng = np.random.default_rng(1000 * n + bits)
    for density in (0.3, 0.6):
        B = unpack(random_rows(rng, n, bits, density))
        counts = B.sum(axis=0, dtype=np.uint64)
        assert counts.max() > 0
        for index in (TAN, RR, SM):
            want = brute(B, index)
            assert 0.0 < want < 1.0
            assert same_double(capi.isim(counts, n, index), want), (n, bits, density, index)
            assert same_double(from_counts(counts, n, index), want)


def test_small_sets_and_all_zero_rows_give_zero():
    counts = np.zeros(64, np.uint64)
    for index in (TAN, RR, SM):
        assert capi.isim(counts, 0, index) == 0.0
    assert capi.isim(np.ones(64, np.uint64), 1, TAN) == 0.0 and capi.isim(np.ones(64, np.uint64), 1, SM) == 0.0
    assert capi.isim(counts, 1, SM) == 0.0
    assert capi.isim(counts, 40, TAN) == 0.0, "0 / 0 counts as 0.0"
    assert capi.isim(counts, 40, RR) == 0.0 and capi.isim(counts, 40, SM) == 1.0


def test_the_128_bit_path_at_the_largest_table():
    n = 2**32 - 1
    counts = np.array([0, 1, n // 2, n - 1, n] * 820, np.uint64)[:4096]
    assert len(counts) == 4096
    a = sum(int(c) * (int(c) - 1) // 2 for c in counts)
    d = sum((n - int(c)) * (n - int(c) - 1) // 2 for c in counts)
    assert a > 2**64 and d > 2**64 and a + d + sum(int(c) * (n - int(c)) for c in counts) > 2**74
    for index in (TAN, RR, SM):
        assert same_double(capi.isim(counts, n, index), from_counts(counts, n, index)), index
    full = np.full(4096, n, np.uint64)
    assert capi.isim(full, n, TAN) == 1.0 and capi.isim(full, n, SM) == 1.0


def test_complement_equals_isim_without_each_row_and_finds_the_medoid():
    rng = np.random.default_rng(300)
    n, bits = 300, 256
    rows = random_rows(rng, n, bits, 0.2)
    rows[7] = 0
    rows[8] = 0xFFFFFFFF
    B = unpack(rows).astype(np.int64)
    counts = B.sum(axis=0).astype(np.uint64)
    sums = (B * counts.astype(np.int64)).sum(axis=1).astype(np.uint64)
    popc = B.sum(axis=1).astype(np.uint32)
    for index in (TAN, RR, SM):
        got = capi.isim_complement(counts, n, sums, popc, index)
        want = np.array([capi.isim(counts - B[i].astype(np.uint64), n - 1, index) for i in range(n)])
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), index
    # the medoid by brute force: the row whose removal leaves the lowest ratio of pair sums
    ones = B @ B.T
    union = popc[:, None].astype(np.int64) + popc[None, :].astype(np.int64) - ones
    np.fill_diagonal(ones, 0)
    np.fill_diagonal(union, 0)
    A, U = int(ones.sum()) // 2, int(union.sum()) // 2
    left = [(A - int(ones[i].sum())) / (U - int(union[i].sum())) for i in range(n)]
    got = capi.isim_complement(counts, n, sums, popc, TAN)
    assert int(np.argmin(got)) == int(np.argmin(left))
    assert np.array_equal(got.view(np.uint64), np.array(left).view(np.uint64))
    assert len(capi.isim_complement(counts, n, [], [], TAN)) == 0
    two = capi.isim_complement(np.array([2, 1], np.uint64), 2, [3, 2], [2, 1], SM)
    assert two.tolist() == [0.0, 0.0], "one row left: no pairs"


def test_invalid_arguments_of_the_host_functions():
    L = capi.load()
    v = C.c_double(7.0)
    counts = np.array([4, 0, 5, 2], np.uint64)
    cp = counts.ctypes.data_as(U64P)
    assert L.gsim_isim(cp, 4, 5, TAN, C.byref(v)) == OK
    cases = {
        "NULL counts": (None, 4, 5, TAN, C.byref(v)), "NULL value": (cp, 4, 5, TAN, None), "fp_bits == 0": (cp, 0, 5, TAN, C.byref(v)),
        "a count above n": (cp, 4, 4, TAN, C.byref(v)), "n == 2^32": (cp, 4, 2**32, TAN, C.byref(v)), "an unknown index": (cp, 4, 5, 3, C.byref(v)),
        "a negative index": (cp, 4, 5, -1, C.byref(v)),
    }
    for what, args in cases.items():
        assert L.gsim_isim(*args) == INVALID and len(message()) > 0, what
    for what, (c, n, index) in {"a count above n": (counts, 4, TAN), "n == 2^32": (counts, 2**32, TAN), "an unknown index": (counts, 5, 9)}.items():
        with pytest.raises(capi.GsimError) as e:
            capi.isim(c, n, index)
        assert e.value.code == INVALID, what
    with pytest.raises(capi.GsimError):
        capi.isim([], 5, TAN)
    # the complement: a row of the set {0b1101, 0b0101, 0b0100, 0b0101, 0b1101} (bit 0 first): counts 4, 0, 5, 2
    sums = np.array([11, 9, 5], np.uint64)
    popc = np.array([3, 2, 1], np.uint32)
    out = np.zeros(3)
    sp, pp, op = sums.ctypes.data_as(U64P), popc.ctypes.data_as(C.POINTER(C.c_uint32)), out.ctypes.data_as(C.POINTER(C.c_double))
    assert L.gsim_isim_complement(cp, 4, 5, TAN, sp, pp, 3, op) == OK
    bad_popc = np.array([3, 5, 1], np.uint32)
    for what, args in {
        "NULL counts": (None, 4, 5, TAN, sp, pp, 3, op), "fp_bits == 0": (cp, 0, 5, TAN, sp, pp, 3, op), "a count above n": (cp, 4, 4, TAN, sp, pp, 3, op),
        "n == 2^32": (cp, 4, 2**32, TAN, sp, pp, 3, op), "an unknown index": (cp, 4, 5, 3, sp, pp, 3, op), "NULL sums": (cp, 4, 5, TAN, None, pp, 3, op),
        "NULL popc": (cp, 4, 5, TAN, sp, None, 3, op), "NULL out": (cp, 4, 5, TAN, sp, pp, 3, None),
        "popc above fp_bits": (cp, 4, 5, TAN, sp, bad_popc.ctypes.data_as(C.POINTER(C.c_uint32)), 3, op),
    }.items():
        assert L.gsim_isim_complement(*args) == INVALID and len(message()) > 0, what
    assert L.gsim_isim_complement(cp, 4, 5, TAN, None, None, 0, None) == OK, "no rows: legal"
    with pytest.raises(capi.GsimError) as e:
        capi.isim_complement(counts, 5, [11, 9], [3, 9], TAN)
    assert e.value.code == INVALID


def test_the_device_calls_on_a_table_that_is_not_on_a_gpu():
    L = capi.load()
    t = capi.Table(1024).add_rows(np.arange(40 * 32, dtype=np.uint32).reshape(40, 32))
    other = capi.Table(1024).add_rows(np.ones((4, 32), np.uint32))
    counts = np.zeros(1024, np.uint64)
    counted = C.c_uint64(9)
    cp = counts.ctypes.data_as(U64P)
    weights = np.ones(1024, np.uint32)
    wp = weights.ctypes.data_as(C.POINTER(C.c_uint32))
    sums = np.zeros(40, np.uint64)
    sp = sums.ctypes.data_as(U64P)
    for what, args in {"NULL db": (None, None, 0, 40, cp, None, None), "NULL counts": (t._h, None, 0, 40, None, None, None),
                       "begin past end": (t._h, None, 5, 4, cp, None, None), "end past the table": (t._h, None, 0, 41, cp, None, None)}.items():
        assert L.gsim_db_bit_counts(*args) == INVALID and len(message()) > 0, what
    assert L.gsim_db_bit_counts(t._h, None, 0, 40, cp, C.byref(counted), None) == STATE and "GPU" in message() and counted.value == 0
    assert L.gsim_db_bit_counts(t._h, None, 3, 3, cp, None, None) == STATE, "an empty range still needs a table on a GPU"
    for what, args in {"NULL db": (None, wp, 0, 40, sp, None, None), "NULL weights": (t._h, None, 0, 40, sp, None, None),
                       "NULL sums": (t._h, wp, 0, 40, None, None, None), "begin past end": (t._h, wp, 5, 4, sp, None, None),
                       "end past the table": (t._h, wp, 0, 41, sp, None, None)}.items():
        assert L.gsim_db_overlap_sums(*args) == INVALID and len(message()) > 0, what
    assert L.gsim_db_overlap_sums(t._h, wp, 0, 40, sp, None, None) == STATE and "GPU" in message()
    for call in (lambda: t.bit_counts(), lambda: t.overlap_sums(weights), lambda: t.overlap_sums(weights, popc=True)):
        with pytest.raises(capi.GsimError) as e:
            call()
        assert e.value.code == STATE
    # the wrapper narrows the weights and refuses what does not fit 32 bits
    for bad in (np.full(1024, 2**32, np.uint64), np.full(1024, -1, np.int64), np.ones(1000, np.uint32), np.ones(1024, np.float64)):
        with pytest.raises(capi.GsimError) as e:
            t.overlap_sums(bad)
        assert e.value.code == INVALID
    wide = capi.Table(4128).add_rows(np.ones((3, 129), np.uint32))
    wc = np.zeros(4128, np.uint64)
    assert L.gsim_db_bit_counts(wide._h, None, 0, 3, wc.ctypes.data_as(U64P), None, None) == INVALID and "4096" in message()
    empty = capi.Table(1024)
    counts[:] = 5
    assert L.gsim_db_bit_counts(empty._h, None, 0, 0, cp, C.byref(counted), None) == OK and not counts.any() and counted.value == 0
    c, n = empty.bit_counts()
    assert n == 0 and not c.any() and len(empty.overlap_sums(weights)) == 0
    for x in (t, other, wide, empty):
        x.close()
