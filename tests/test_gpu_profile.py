"""Per-bit column counts and weighted popcounts on the GPU (gsim_db_bit_counts, gsim_db_overlap_sums) and, end to end, the iSIM index
and the medoid they lead to.

Expected values come from numpy on the host rows, never from the library: np.unpackbits(rows.view(np.uint8), bitorder="little") and
integer sums (uint64 throughout: the largest sum, 4096 x (2^32 - 1), fits).  Every comparison is exact.

The parity tables are 5 000 rows of 32, 96, 160, 1024, 2048, 2080 and 4096 bits (2080 bits = 65 words: the only width here at which a
lane of the VALU kernel of gsim_db_overlap_sums owns two words and a workgroup of the counting kernel holds three row lanes), of the
sparse, dense and Morgan kinds, each with a planted all-zero row, an all-ones row and seven identical rows.  Asserted on the EXPECTED
result before anything is compared: every column count is non-zero and at least two columns differ."""
import contextlib
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from gpusimilarity_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 5000
WIDTHS = [32, 96, 160, 1024, 2048, 2080, 4096]
KINDS = {"sparse": O.KIND_SPARSE, "dense": O.KIND_DENSE, "morgan": O.KIND_MORGAN}
GATHER_KNOB, LAUNCH_KNOB = "GSIM_SUBSET_GATHER_MAX_PERMILLE", "GSIM_PROFILE_LAUNCH_ROWS"
STREAM, GATHER = "0", "1000"  # values of the route knob that force either route
ZERO_ROW, ONES_ROW, COPIES = N // 2, N // 2 + 1, range(N // 3, N // 3 + 6)


@contextlib.contextmanager
def knobs(**values):
    """The knobs are read once per handle, by gsim_db_create: set them around the creation of a table."""
    old = {k: os.environ.get(k) for k in values}
    for k, v in values.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make_table(db, gather=None, launch_rows=None):
    with knobs(**{GATHER_KNOB: gather, LAUNCH_KNOB: launch_rows}):
        return capi.Table(db.shape[1] * 32).add_rows(db).finalize(0, 1)


def unpack(rows):
    rows = np.ascontiguousarray(rows)
    return np.unpackbits(rows.view(np.uint8), bitorder="little").reshape(len(rows), rows.shape[1] * 32)


def counts_of(rows):
    return unpack(rows).sum(axis=0, dtype=np.uint64)


def sums_of(rows, weights):
    return unpack(rows).astype(np.uint64) @ np.asarray(weights, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def planted(bits, kind):
    """the host rows of a parity table (computed once, never modified)"""
    db = O.synth_rows(0x150 + bits, KINDS[kind], 0, N, bits // 32)
    for r in COPIES:
        db[r] = db[5]
    db[ZERO_ROW] = 0
    db[ONES_ROW] = 0xFFFFFFFF
    db.setflags(write=False)
    return db


@functools.lru_cache(maxsize=None)
def expected(bits, kind):
    """(counts uint64 [bits], popc uint32 [N]) of a parity table, from numpy"""
    B = unpack(planted(bits, kind))
    counts, popc = B.sum(axis=0, dtype=np.uint64), B.sum(axis=1, dtype=np.uint32)
    assert counts.min() > 0 and len(np.unique(counts)) >= 2, "the expected result is not vacuous"
    assert popc[ZERO_ROW] == 0 and popc[ONES_ROW] == bits
    counts.setflags(write=False)
    return counts, popc


_tables = {}


def parity_table(bits, kind):
    """the table of a parity case on the GPU with the default knobs, shared by the tests of this module"""
    if (bits, kind) not in _tables:
        _tables[(bits, kind)] = make_table(planted(bits, kind))
    return _tables[(bits, kind)]


@pytest.fixture(scope="module", autouse=True)
def close_tables():
    yield
    for t in _tables.values():
        t.close()
    _tables.clear()


CASES = [(b, k) for b in WIDTHS for k in KINDS]


@pytest.mark.parametrize("bits,kind", CASES)
def test_bit_counts_parity(bits, kind):
    want, _ = expected(bits, kind)
    st = {}
    counts, counted = parity_table(bits, kind).bit_counts(stats=st)
    assert counts.dtype == np.uint64 and np.array_equal(counts, want)
    assert counted == N and st["rows_counted"] == N and st["rows_read"] == N
    assert st["route"] == capi.PROFILE_STREAMED and st["launches"] == 1 and st["kernel_ms"] > 0 and st["wall_ms"] > 0


def test_carry_chains_all_ones():
    """every counter past 2^16, all planes of every word carry at once; then the sizes around a step of the workgroup (256-bit rows:
    two chunks per row, 128 row lanes, eight rows per thread and step)"""
    n = 70001
    db = np.full((n, 8), 0xFFFFFFFF, np.uint32)
    t = make_table(db)
    counts, counted = t.bit_counts()
    assert counted == n and (counts == n).all() and n > 2**16
    for a, b in ((0, 65536), (1, 65538), (69000, n)):
        assert (t.bit_counts(row_begin=a, row_end=b)[0] == b - a).all()
    t.close()
    for small in (1, 2, 255, 256, 257, 1023, 1024, 1025):
        t = make_table(db[:small])
        counts, counted = t.bit_counts()
        assert counted == small and (counts == small).all(), small
        t.close()


@pytest.mark.parametrize("bits", [160, 1024])
def test_ranges(bits):
    db, t = planted(bits, "morgan"), parity_table(bits, "morgan")
    for a, b in ((1, N - 3), (0, 1), (N - 1, N), (ZERO_ROW, ZERO_ROW + 2), (257, 4099)):
        counts, counted = t.bit_counts(row_begin=a, row_end=b)
        assert counted == b - a and np.array_equal(counts, counts_of(db[a:b])), (a, b)
    counts, counted = t.bit_counts(row_begin=7, row_end=7)
    assert counted == 0 and not counts.any(), "an empty range: zeros"
    st = {}
    t.bit_counts(row_begin=N, row_end=N, stats=st)
    assert st["launches"] == 0 and st["route"] == 0
    cuts = [0, 1237, 1238, N]
    pieces = [t.bit_counts(row_begin=a, row_end=b) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(sum(p[0] for p in pieces), expected(bits, "morgan")[0]) and sum(p[1] for p in pieces) == N
    with pytest.raises(capi.GsimError) as e:
        t.bit_counts(row_begin=0, row_end=N + 1)
    assert e.value.code == -1
    with pytest.raises(capi.GsimError) as e:
        t.bit_counts(row_begin=5, row_end=4)
    assert e.value.code == -1


@pytest.mark.parametrize("route", [STREAM, GATHER])
@pytest.mark.parametrize("bits", [160, 1024])
def test_row_sets(bits, route):
    db = planted(bits, "sparse")
    t = make_table(db, gather=route)
    want_route = capi.PROFILE_GATHERED if route == GATHER else capi.PROFILE_STREAMED
    rng = np.random.default_rng(bits)
    picks = {"1 %": rng.choice(N, N // 100, replace=False), "60 %": rng.choice(N, N * 6 // 10, replace=False),
             "one row": np.array([N - 1]), "a run": np.arange(1000, 1300)}
    for what, rows in picks.items():
        rows = np.sort(rows)
        rs = t.rowset(rows=rows.astype(np.uint32))
        st = {}
        counts, counted = t.bit_counts(rs, stats=st)
        assert counted == len(rows) and np.array_equal(counts, counts_of(db[rows])), what
        assert st["route"] == want_route and st["rows_read"] == (len(rows) if route == GATHER else N), what
        # the set intersected with ranges, unaligned ones and one that holds none of it
        for a, b in ((1, N - 3), (1237, 1238), (1000, 1100), (0, int(rows[0]))):
            inside = rows[(rows >= a) & (rows < b)]
            counts, counted = t.bit_counts(rs, row_begin=a, row_end=b)
            assert counted == len(inside) and np.array_equal(counts, counts_of(db[inside])), (what, a, b)
        rs.close()
    # an exclusion set: everything but the 60 %
    rows = np.sort(picks["60 %"])
    rs = t.rowset(rows=rows.astype(np.uint32), exclude=True)
    rest = np.setdiff1d(np.arange(N), rows)
    counts, counted = t.bit_counts(rs)
    assert counted == len(rest) == N - len(rows) and np.array_equal(counts, counts_of(db[rest]))
    rs.close()
    # the empty set, and a bitmap
    rs = t.rowset(rows=np.zeros(0, np.uint32))
    st = {}
    counts, counted = t.bit_counts(rs, stats=st)
    assert counted == 0 and not counts.any() and st["launches"] == 0
    rs.close()
    bitmap = rng.integers(0, 2**32, (N + 31) // 32, dtype=np.uint64).astype(np.uint32)
    rs = t.rowset(bitmap=bitmap)
    chosen = np.nonzero(np.unpackbits(bitmap.view(np.uint8), bitorder="little")[:N])[0]
    counts, counted = t.bit_counts(rs)
    assert counted == len(chosen) and np.array_equal(counts, counts_of(db[chosen]))
    rs.close()
    # a row base plays no part: the set's rows carry it, the range and the result do not
    t.set_row_base(1000)
    rs = t.rowset(rows=(np.arange(10, 20) + 1000).astype(np.uint32))
    counts, counted = t.bit_counts(rs, row_begin=12, row_end=N)
    assert counted == 8 and np.array_equal(counts, counts_of(db[12:20]))
    rs.close()
    t.close()


def test_the_default_rule_is_that_of_row_set_searches():
    """a 1 % set gathers, a 60 % set streams (GSIM_SUBSET_GATHER_MAX_PERMILLE's default: a quarter of the table's bytes)"""
    db, t = planted(1024, "sparse"), parity_table(1024, "sparse")
    for share, want in ((100, capi.PROFILE_GATHERED), (2, capi.PROFILE_STREAMED)):
        rows = np.arange(0, N, share, dtype=np.uint32)
        rs = t.rowset(rows=rows)
        st = {}
        counts, counted = t.bit_counts(rs, stats=st)
        assert st["route"] == want and counted == len(rows) and np.array_equal(counts, counts_of(db[rows]))
        rs.close()
    other = make_table(db[:64])
    rs = other.rowset(rows=np.arange(4, dtype=np.uint32))
    with pytest.raises(capi.GsimError) as e:
        t.bit_counts(rs)
    assert e.value.code == -1, "a set of another handle"
    rs.close()
    other.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_generated_tables(kind):
    seed = 0x6E4 + KINDS[kind]
    t = capi.Table(1024).generate(seed, KINDS[kind], 0, N)
    db = O.synth_rows(seed, KINDS[kind], 0, N, 32)
    counts, counted = t.bit_counts()
    want = counts_of(db)
    assert counted == N and want.max() > 0 and np.array_equal(counts, want)
    sums, popc = t.overlap_sums(counts, popc=True)
    assert np.array_equal(sums, sums_of(db, want)) and np.array_equal(popc, unpack(db).sum(axis=1, dtype=np.uint32))
    t.close()


@pytest.mark.parametrize("bits", [160, 1024])
def test_launch_cuts_do_not_change_a_byte(bits):
    db = planted(bits, "dense")
    whole, cut = parity_table(bits, "dense"), make_table(db, launch_rows=256)
    weights = np.random.default_rng(bits).integers(0, 2**32, bits, dtype=np.uint64)
    rows = np.sort(np.random.default_rng(1).choice(N, 3000, replace=False)).astype(np.uint32)
    sa, sb = {}, {}
    a, b = whole.bit_counts(stats=sa), cut.bit_counts(stats=sb)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] == N
    assert sa["launches"] == 1 and sb["launches"] == (N + 255) // 256
    for gather in (STREAM, GATHER):
        t2 = make_table(db, gather=gather, launch_rows=256)
        rs, rs2 = whole.rowset(rows=rows), t2.rowset(rows=rows)
        st = {}
        a, b = whole.bit_counts(rs, row_begin=3, row_end=N - 5), t2.bit_counts(rs2, row_begin=3, row_end=N - 5, stats=st)
        assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
        assert st["launches"] > 1
        rs.close()
        rs2.close()
        t2.close()
    sa, sb = {}, {}
    a, b = whole.overlap_sums(weights, 3, N - 5, popc=True, stats=sa), cut.overlap_sums(weights, 3, N - 5, popc=True, stats=sb)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert np.array_equal(a[0], sums_of(db[3:N - 5], weights))
    assert sa["launches"] == 1 and sb["launches"] == (N - 8 + 255) // 256
    cut.close()


def test_the_search_state_is_left_as_found():
    db, t = planted(1024, "morgan"), parity_table(1024, "morgan")
    q = db[[5, 77, ONES_ROW]]
    before = t.search(q, 50, 0.1)
    counts, _ = t.bit_counts()
    rs = t.rowset(rows=np.arange(0, N, 3, dtype=np.uint32))
    t.bit_counts(rs)
    t.overlap_sums(counts, popc=True)
    rs.close()
    after = t.search(q, 50, 0.1)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before[0], after[0])) and before[1].tobytes() == after[1].tobytes()
    want, wap = O.search(q[0], db, 50, 0.1, nthreads=4)
    assert np.array_equal(after[0][0]["row"], want["row"]) and int(after[1][0]) == wap


@pytest.mark.parametrize("bits,kind", CASES)
def test_overlap_sums_parity(bits, kind):
    db, t = planted(bits, kind), parity_table(bits, kind)
    counts, popc = expected(bits, kind)
    want_route = capi.PROFILE_STREAMED | (capi.PROFILE_MATRIX if bits % 256 == 0 else capi.PROFILE_VALU)
    # the table's own counts: S_i, the row's total overlap with the table
    st = {}
    sums, pc = t.overlap_sums(counts, popc=True, stats=st)
    assert sums.dtype == np.uint64 and pc.dtype == np.uint32
    assert np.array_equal(sums, sums_of(db, counts)) and np.array_equal(pc, popc)
    assert sums[ZERO_ROW] == 0 and sums[ONES_ROW] == counts.sum() and len(set(sums[list(COPIES)].tolist())) == 1
    assert st["route"] == want_route and st["rows_read"] == N and st["launches"] == 1
    # random 32-bit weights (asymmetric: a swapped plane or row would show), without popc
    weights = np.random.default_rng(bits * 3 + KINDS[kind]).integers(0, 2**32, bits, dtype=np.uint64)
    assert np.array_equal(t.overlap_sums(weights), sums_of(db, weights))
    # ... and weights of few planes
    small = weights % 200
    assert np.array_equal(t.overlap_sums(small), sums_of(db, small))


@pytest.mark.parametrize("bits", [96, 160, 2080, 4096])
def test_overlap_sums_extremes(bits):
    db, t = planted(bits, "dense"), parity_table(bits, "dense")
    _, popc = expected(bits, "dense")
    top = np.full(bits, 0xFFFFFFFF, np.uint64)
    sums = t.overlap_sums(top)
    assert np.array_equal(sums, popc.astype(np.uint64) * np.uint64(0xFFFFFFFF))
    assert int(sums[ONES_ROW]) == bits * (2**32 - 1) and int(sums.max()) == int(sums[ONES_ROW]), "the largest sum there is"
    high = t.overlap_sums(np.full(bits, 2**31, np.uint64))
    assert np.array_equal(high, popc.astype(np.uint64) << np.uint64(31)), "a single high plane"
    zero, pc = t.overlap_sums(np.zeros(bits, np.uint32), popc=True)
    assert not zero.any() and np.array_equal(pc, popc), "all-zero weights still give the popcounts"
    one = np.zeros(bits, np.uint64)
    one[bits - 1] = 2**32 - 1
    one[0] = 1
    assert np.array_equal(t.overlap_sums(one), sums_of(db, one)), "the first and the last column"


@pytest.mark.parametrize("bits", [160, 1024])
def test_overlap_sums_ranges(bits):
    db, t = planted(bits, "sparse"), parity_table(bits, "sparse")
    weights = np.random.default_rng(7).integers(0, 2**32, bits, dtype=np.uint64)
    want, (_, popc) = sums_of(db, weights), expected(bits, "sparse")
    for a, b in ((1, N - 3), (0, 1), (N - 1, N), (31, 65), (1237, 1238)):
        sums, pc = t.overlap_sums(weights, a, b, popc=True)
        assert len(sums) == b - a and np.array_equal(sums, want[a:b]) and np.array_equal(pc, popc[a:b]), (a, b)
    assert len(t.overlap_sums(weights, 9, 9)) == 0
    with pytest.raises(capi.GsimError) as e:
        t.overlap_sums(weights, 0, N + 1)
    assert e.value.code == -1


def test_valu_kernel_at_the_matrix_widths_and_multi_shard_handles():
    """The test-hooks build, GSIM_TEST_PROFILE_VALU = 1: the VALU kernel of gsim_db_overlap_sums at widths the matrix cores take
    otherwise -- both kernels must give the same bytes as numpy.  And two logical devices on one GPU: a state error."""
    from conftest import hooks_env, HOOKS_LIB
    assert os.path.exists(HOOKS_LIB)
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import numpy as np, oracle_lib as O; from gpusimilarity_amd import capi\n"
            "for bits in (256, 1024, 4096):\n"
            "    db = O.synth_rows(0x77 + bits, O.KIND_MORGAN, 0, 3001, bits // 32)\n"
            "    db[17] = 0xFFFFFFFF\n"
            "    B = np.unpackbits(db.view(np.uint8), bitorder='little').reshape(len(db), -1).astype(np.uint64)\n"
            "    w = np.random.default_rng(bits).integers(0, 2**32, bits, dtype=np.uint64)\n"
            "    t = capi.Table(bits).add_rows(db).finalize(0, 1)\n"
            "    st = {}\n"
            "    sums, pc = t.overlap_sums(w, 1, 3000, popc=True, stats=st)\n"
            "    assert st['route'] == capi.PROFILE_STREAMED | capi.PROFILE_VALU, st\n"
            "    assert np.array_equal(sums, (B @ w)[1:3000]) and np.array_equal(pc, B.sum(axis=1)[1:3000].astype(np.uint32)), bits\n"
            "    t.close()\n"
            "print('valu ok')\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=hooks_env(GSIM_TEST_PROFILE_VALU="1"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "valu ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    code = ("import sys; sys.path.insert(0, %r); import numpy as np; from gpusimilarity_amd import capi\n"
            "t = capi.Table(1024).add_rows(np.ones((512, 32), np.uint32)).finalize(0, 2)\n"
            "assert t.shard_count() == 2\n"
            "for call in (lambda: t.bit_counts(), lambda: t.overlap_sums(np.ones(1024, np.uint32))):\n"
            "    try:\n        call()\n    except capi.GsimError as e:\n        print('code', e.code)\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=hooks_env(GSIM_TEST_ALIAS_DEVICES="2"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.count("code -5") == 2, r.stdout + r.stderr


def test_end_to_end_isim_and_the_medoid():
    """400 rows: the GPU's counts -> isim == the brute-force ratio of pair sums; the GPU's sums and popcounts -> isim_complement, whose
    argmin is the brute-force medoid (the row whose removal leaves the lowest ratio) and whose argmax is the brute-force outlier."""
    n, bits = 400, 1024
    db = O.synth_rows(0xE2E, O.KIND_MORGAN, 0, n, bits // 32).copy()
    db[123] = O.synth_rows(0xBAD, O.KIND_DENSE, 0, 1, bits // 32)[0]  # a dense row among Morgan rows
    t = make_table(db)
    counts, counted = t.bit_counts()
    sums, popc = t.overlap_sums(counts, popc=True)
    t.close()
    B = unpack(db).astype(np.int64)
    ones = B @ B.T
    pops = B.sum(axis=1)
    union = pops[:, None] + pops[None, :] - ones
    iu = np.triu_indices(n, 1)
    A, U = int(ones[iu].sum()), int(union[iu].sum())
    assert counted == n and 0 < A < U
    assert capi.isim(counts, n, capi.ISIM_TANIMOTO) == float(A) / float(U)
    zeros = (1 - B) @ (1 - B).T
    D = int(zeros[iu].sum())
    P = len(iu[0]) * bits
    assert capi.isim(counts, n, capi.ISIM_RUSSELL_RAO) == float(A) / float(P)
    assert capi.isim(counts, n, capi.ISIM_SIMPLE_MATCHING) == float(A + D) / float(P)
    np.fill_diagonal(ones, 0)
    np.fill_diagonal(union, 0)
    left = np.array([float(A - int(ones[i].sum())) / float(U - int(union[i].sum())) for i in range(n)])
    comp = capi.isim_complement(counts, n, sums, popc, capi.ISIM_TANIMOTO)
    assert np.array_equal(comp.view(np.uint64), left.view(np.uint64))
    assert int(np.argmin(comp)) == int(np.argmin(left)) and len(np.unique(left)) > n // 2
    assert int(np.argmax(comp)) == int(np.argmax(left))
