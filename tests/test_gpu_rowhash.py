"""gsim_rowhash_* on the GPU against the numpy restatement of the rule (rowhash_rule.py): the duplicate groups, the stats, both row
sets and the slot count byte for byte at every kernel instantiation; the edges of a wave's and a workgroup's rows; tables of identical
and of all-zero rows; probe chains that wrap at the table's end and chains of 200 rows with one first slot; rows one bit apart;
lookups of host rows and of another table's rows; the representatives' row set under gsim_db_search_rows; a generated Morgan table;
an attached tensor; determinism, the search state, a changed table and the destroy order."""
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import rowhash_rule as R
from gpusimilarity_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE = -1, -5
# 32 .. 192, 448, 896: one row per lane; 128 .. 8192 by powers of two: 1 .. 64 lanes per row; 1152, 32768: one row per wave
WIDTHS = [32, 64, 96, 160, 192, 448, 896, 1024, 1152, 2048, 4096, 32768]
MORE_WIDTHS = [128, 256, 512, 8192]  # the other instantiations of the sixteen-byte kernel


def kernel_constants():
    text = open(os.path.join(ROOT, "gpusimilarity_amd", "csrc", "gsim_device.h")).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % n, text).group(1)) for n in ("kRowhashBlock", "kRowhashUnroll"))


BLOCK, UNROLL = kernel_constants()
WAVE_ROWS = 64                  # rows of a wave's trip at one row per lane, and of the finishing pass
WORKGROUP_ROWS = BLOCK          # ... of a workgroup's


def chunk_rows(bits):
    """rows of one wave's chunk in the inserting pass (gsim_device.h)"""
    W = bits // 32
    if W % 4 == 0 and (W // 4) & (W // 4 - 1) == 0 and W // 4 <= 64:
        return UNROLL * 64 // (W // 4)
    return 64 if W < 32 else 1


def table(db, base=0):
    t = capi.Table(db.shape[1] * 32).add_rows(db).finalize(0, 1)
    if base:
        t.set_row_base(base)
    return t


def random_rows(rng, n, W):
    return rng.integers(0, 2 ** 32, (n, W), dtype=np.uint32) & rng.integers(0, 2 ** 32, (n, W), dtype=np.uint32)


def planted(rng, n, W, sizes=(2, 3, 64, 1000), chunk=1):
    """n random rows with groups of `sizes` identical rows scattered over the table; the first group's lowest row is the last row
    of a chunk and its other members lie behind it"""
    db = random_rows(rng, n, W)
    free = rng.permutation(np.arange(chunk, n))  # (the rows behind the first chunk)
    db[free[:sizes[0] - 1]] = db[chunk - 1]
    at = sizes[0] - 1
    for size in sizes[1:]:
        db[free[at:at + size]] = db[free[at]]
        at += size
    return db


def check(t, db, base=0, what=""):
    """everything the index shows equals the rule"""
    first, size, counts = R.groups(db, base)
    n = len(db)
    with t.rowhash() as ix:
        f, s = ix.groups()
        assert f.dtype == np.uint32 and s.dtype == np.uint32
        assert f.tobytes() == first.tobytes(), (what, np.flatnonzero(f != first)[:5])
        assert s.tobytes() == size.tobytes(), (what, np.flatnonzero(s != size)[:5])
        st = ix.stats()
        assert {k: st[k] for k in counts} == counts, (what, st, counts)
        assert st["launches"] == (3 if n else 0)
        reps = np.flatnonzero(first == np.arange(n, dtype=np.uint32) + np.uint32(base)).astype(np.uint32) + np.uint32(base)
        others = np.setdiff1d(np.arange(n, dtype=np.uint32) + np.uint32(base), reps)
        if n:  # (a row set needs rows on a GPU; an empty table has them too, but nothing to select)
            for repeats, want in ((False, reps), (True, others)):
                rs = ix.rowset(repeats=repeats)
                assert rs.count == len(want) and rs.rows().tobytes() == want.astype(np.uint32).tobytes(), (what, repeats)
                rs.close()
            assert len(reps) == st["groups"]
    return first, size, counts


# ---- the groups ----

@pytest.mark.parametrize("bits", WIDTHS + MORE_WIDTHS)
def test_groups_stats_row_sets_and_slots_equal_the_rule(bits):
    rng = np.random.default_rng(0xD0 + bits)
    W, n = bits // 32, 5000
    db = planted(rng, n, W, chunk=chunk_rows(bits))
    first, size, counts = R.groups(db)
    assert counts["largest_group"] >= 1000 and counts["repeated_groups"] >= 4 and counts["slots"] == 16384
    lowest = chunk_rows(bits) - 1
    assert first[lowest] == lowest and size[lowest] == 2 and int(np.flatnonzero(first == lowest)[1]) > lowest
    t = table(db, base=77)
    check(t, db, 77, bits)
    t.close()


@pytest.mark.parametrize("n", [0, 1, WAVE_ROWS - 1, WAVE_ROWS, WAVE_ROWS + 1, WORKGROUP_ROWS - 1, WORKGROUP_ROWS, WORKGROUP_ROWS + 1])
def test_the_edges_of_a_waves_and_a_workgroups_rows(n):
    """32 and 160 bits: 64 rows per wave trip, 256 per workgroup; 1024 bits: chunks of 32 rows; 1152 bits: a row per wave -- and the
    finishing pass of every width: 64 rows per wave, 256 per workgroup"""
    assert (WAVE_ROWS, WORKGROUP_ROWS) == (64, 256) and chunk_rows(32) == 64 and chunk_rows(1024) == 32 and chunk_rows(1152) == 1
    for bits in (32, 160, 1024, 1152):
        rng = np.random.default_rng(n * 7 + bits)
        db = random_rows(rng, n, bits // 32)
        if n >= 2:
            db[n - 1] = db[0]  # the table's last row joins its first
        if n > 70:
            db[[5, 64, 69]] = db[63]
        t = table(db)
        check(t, db, 0, (bits, n))
        with t.rowhash() as ix:
            q = np.concatenate([db, random_rows(rng, 3, bits // 32) | np.uint32(1 << 31)])
            row, size = ix.find(q)
            wrow, wsize = R.find(db, q)
            assert row.tobytes() == wrow.tobytes() and size.tobytes() == wsize.tobytes(), (bits, n)
        t.close()


def test_identical_rows_and_zero_rows():
    W = 32
    same = np.tile(O.synth_rows(7, O.KIND_MORGAN, 0, 1, W), (4096, 1))
    t = table(same)
    _, _, counts = check(t, same, 0, "identical")
    assert counts["groups"] == 1 and counts["largest_group"] == 4096 and counts["repeated_groups"] == 1
    t.close()
    for bits in (64, 1024, 1152):
        zeros = np.zeros((300, bits // 32), np.uint32)
        t = table(zeros, base=5)
        first, size, counts = check(t, zeros, 5, "zeros")
        assert (first == 5).all() and (size == 300).all() and counts["groups"] == 1
        t.close()
        rng = np.random.default_rng(bits)
        mixed = random_rows(rng, 1000, bits // 32)
        mixed[[3, 900]] = mixed[17]
        mixed[np.setdiff1d(rng.permutation(1000)[:130], [3, 17, 900])[:120]] = 0
        t = table(mixed)
        first, size, _ = check(t, mixed, 0, "mixed")
        z = np.flatnonzero(~mixed.any(axis=1))
        assert len(z) >= 120 and (first[z] == z[0]).all() and (size[z] == len(z)).all()
        with t.rowhash() as ix:
            row, sz = ix.find(np.zeros((1, bits // 32), np.uint32))
            assert row[0] == z[0] and sz[0] == len(z), "an all-zero query finds the all-zero rows"
        t.close()


# ---- adversarial probing ----

@pytest.mark.parametrize("bits", [1024, 160, 1152])
def test_chains_that_wrap_at_the_last_slot_and_200_rows_with_one_first_slot(bits):
    rng = np.random.default_rng(0xADD + bits)
    W, n = bits // 32, 500
    assert R.slots(n) == R.MIN_SLOTS == 1024
    last = R.colliding_rows(rng, n, W, 1023, 80)      # 40 in the table, 40 absent
    middle = R.colliding_rows(rng, n, W, 517, 240)    # 200 in the table, 40 absent
    copies = np.concatenate([np.repeat(np.arange(20), 2), np.repeat(np.arange(20, 40), 3)])
    db = np.concatenate([last[copies], middle[:200]])
    db = np.concatenate([db, random_rows(rng, n - len(db), W)])
    db = db[rng.permutation(n)]
    assert len(db) == n and (R.first_slot(R.row_hash(last), n) == 1023).all() and (R.first_slot(R.row_hash(middle), n) == 517).all()
    t = table(db, base=9)
    first, size, counts = check(t, db, 9, bits)
    assert counts["slots"] == 1024 and counts["repeated_groups"] >= 40
    with t.rowhash() as ix:
        q = np.concatenate([last, middle, db[:50]])
        row, sz = ix.find(q)
        wrow, wsz = R.find(db, q, 9)
        assert row.tobytes() == wrow.tobytes() and sz.tobytes() == wsz.tobytes()
        assert (wrow[40:80] == R.ROW_NONE).all() and (wrow[280:320] == R.ROW_NONE).all() and (wrow[:40] != R.ROW_NONE).all()
        assert sorted(set(wsz[:40].tolist())) == [2, 3]
    t.close()


@pytest.mark.parametrize("bits", [160, 1024, 1152, 2048])
def test_rows_one_bit_apart_are_never_grouped(bits):
    rng = np.random.default_rng(0xB17 + bits)
    W = bits // 32
    base_row = random_rows(rng, 1, W)[0]
    rows = [base_row]
    for word in (0, W - 1):
        for bit in range(32):
            r = base_row.copy()
            r[word] ^= np.uint32(1 << bit)
            rows.append(r)
    db = np.array(rows, np.uint32)
    db = np.concatenate([db, db[[0, 1, 40]]])  # ... and three true repeats
    t = table(db)
    first, size, counts = check(t, db, 0, bits)
    assert counts["groups"] == 65 and counts["repeated_groups"] == 3 and counts["largest_group"] == 2
    t.close()


# ---- lookups ----

@pytest.mark.parametrize("bits", [96, 1024, 1152])
def test_find(bits):
    rng = np.random.default_rng(0xF1 + bits)
    W, n, base = bits // 32, 3000, 4000000000
    db = planted(rng, n, W, sizes=(2, 50))
    db[[10, 2000]] = 0
    t = table(db, base=base)
    with t.rowhash() as ix:
        pool = np.concatenate([db, random_rows(rng, 2000, W) | np.uint32(1), np.zeros((1, W), np.uint32)])
        for nq in (0, 1, 63, 64, 65, 5000):
            q = pool[rng.integers(0, len(pool), nq)]
            row, sz = ix.find(q)
            wrow, wsz = R.find(db, q, base)
            assert row.tobytes() == wrow.tobytes() and sz.tobytes() == wsz.tobytes(), (bits, nq)
            row2, none = ix.find(q, size=False)
            assert none is None and row2.tobytes() == wrow.tobytes()
        wrow, wsz = R.find(db, pool, base)
        assert (wrow == R.ROW_NONE).sum() >= 1900 and wsz.max() == 50 and wrow[wrow != R.ROW_NONE].min() >= base
        assert wrow[-1] == base + 10 and wsz[-1] == 2
    t.close()


def test_find_db():
    rng = np.random.default_rng(0xDB)
    W, n = 32, 2000
    db = planted(rng, n, W, sizes=(2, 30))
    other_rows = np.concatenate([db[rng.integers(0, n, 500)], random_rows(rng, 500, W) | np.uint32(1)])
    other_rows = other_rows[rng.permutation(1000)]
    t, other = table(db, base=100), table(other_rows, base=7)
    first, size, _ = R.groups(db, 100)
    with t.rowhash() as ix:
        row, sz = ix.find_db(other)
        wrow, wsz = R.find(db, other_rows, 100)
        assert row.tobytes() == wrow.tobytes() and sz.tobytes() == wsz.tobytes() and 400 <= (wrow != R.ROW_NONE).sum() <= 600
        row, sz = ix.find_db(other, 123, 457)
        assert row.tobytes() == wrow[123:457].tobytes() and sz.tobytes() == wsz[123:457].tobytes()
        row, sz = ix.find_db(other, 9, 9)
        assert len(row) == 0
        row, sz = ix.find_db(t, 50, 1900)  # the table itself: row == first
        assert row.tobytes() == first[50:1900].tobytes() and sz.tobytes() == size[50:1900].tobytes()
        narrow = table(random_rows(rng, 10, 2))
        for args, code, text in (((narrow,), INVALID, "different fp_bits"), ((other, 0, 1001), INVALID, "outside the left table"),
                                 ((other, 5, 4), INVALID, "begin past end")):
            with pytest.raises(capi.GsimError) as e:
                ix.find_db(*args)
            assert e.value.code == code and text in str(e.value), args
        narrow.close()
        host = capi.Table(W * 32).add_rows(db[:5])
        with pytest.raises(capi.GsimError) as e:
            ix.find_db(host)
        assert e.value.code == STATE
        host.close()
        # another table's index answers for ITS table: the index, not the caller, names the table
        with other.rowhash() as oix:
            row, _ = oix.find_db(t)
            assert row.tobytes() == R.find(other_rows, db, 7)[0].tobytes()
    t.close()
    other.close()


# ---- composition ----

def test_the_representatives_row_set_searches_the_deduplicated_library():
    rng = np.random.default_rng(0xC0)
    W, n, base = 32, 6000, 1000
    db = O.synth_rows(0xC0, O.KIND_MORGAN, 0, n, W)
    db[rng.permutation(n)[:900]] = db[rng.integers(0, n, 900)]
    first, size, counts = R.groups(db, base)
    reps = np.flatnonzero(first == np.arange(n) + base)
    assert counts["groups"] == len(reps) < n - 500
    t, distinct = table(db, base=base), table(db[reps])
    with t.rowhash() as ix:
        rs, rep = ix.rowset(), ix.rowset(repeats=True)
        assert rs.count == ix.stats()["groups"] == len(reps) and rep.count == n - len(reps)
        assert np.array_equal(np.sort(np.concatenate([rs.rows(), rep.rows()])), np.arange(n) + base), "the complement"
        q = db[[5, 700, 4000]]
        for k, cutoff in ((10, 0.0), (300, 0.3)):
            got, gap = t.search_rows(rs, q, k, cutoff)
            want, wap = distinct.search(q, k, cutoff)
            assert gap.tobytes() == wap.tobytes()
            for g, w in zip(got, want):
                w = w.copy()
                w["row"] = (reps[w["row"]] + base).astype(np.uint32)
                assert g.tobytes() == w.tobytes()
        bits, counted = t.bit_counts(rowset=rs)[:2]
        dbits = distinct.bit_counts()[0]
        assert np.array_equal(bits, dbits) and counted == len(reps)
        rs.close()
        rep.close()
    t.close()
    distinct.close()


def test_a_generated_morgan_table_and_an_attached_tensor():
    import torch
    W, n, seed = 32, 200000, 0x30A6
    db = O.synth_rows(seed, O.KIND_MORGAN, 0, n, W)
    first, size, counts = R.groups(db)
    assert (size >= 2).sum() > n // 100, "the generator plants exact duplicates, and the rule finds them"
    g = capi.Table(W * 32).generate(seed, capi.SYNTH_MORGAN, 0, n, 0)
    with g.rowhash() as ix:
        f, s = ix.groups()
        assert f.tobytes() == first.tobytes() and s.tobytes() == size.tobytes()
        st = ix.stats()
        assert {k: st[k] for k in counts} == counts and st["slots"] == 524288
    g.close()
    m = 5000
    ten = torch.from_numpy(db[:m].view(np.int32).copy()).to("cuda:0")
    a = capi.Table(W * 32)
    a.attach_device_rows(ten.data_ptr(), m, 0)
    check(a, db[:m], 0, "attached")
    a.close()
    del ten


# ---- state and lifetime ----

def test_determinism_the_search_state_a_changed_table_and_the_destroy_order():
    rng = np.random.default_rng(0x57)
    n, W = 7003, 32
    db = O.synth_rows(0x57E, O.KIND_MORGAN, 0, n, W)
    db[rng.permutation(n)[:2000]] = db[rng.integers(0, 50, 2000)]  # heavy groups: many rows race for few slots
    t = table(db)
    q = db[[3, 500, 6000]]
    before = [t.search(q[i], k, cut) for i in range(3) for k, cut in ((10, 0.0), (9000, 0.0), (100, 0.4))]
    ix, ix2 = t.rowhash(), t.rowhash()
    (f1, s1), (f2, s2) = ix.groups(), ix2.groups()
    assert f1.tobytes() == f2.tobytes() and s1.tobytes() == s2.tobytes(), "two builds, identical bytes"
    r1, r2 = ix.find(db), ix2.find(db)
    assert r1[0].tobytes() == r2[0].tobytes() == f1.tobytes() and r1[1].tobytes() == r2[1].tobytes() == s1.tobytes()
    a, b = ix.stats(), ix2.stats()
    assert all(a[k] == b[k] for k in ("rows", "groups", "repeated_groups", "largest_group", "slots", "launches"))
    after = [t.search(q[i], k, cut) for i in range(3) for k, cut in ((10, 0.0), (9000, 0.0), (100, 0.4))]
    for (h1, a1), (h2, a2) in zip(before, after):
        assert h1[0].tobytes() == h2[0].tobytes() and a1.tobytes() == a2.tobytes()
    ix.close()
    row, _ = ix2.find(db[:5])  # one index goes, the other still serves
    assert row.tobytes() == f1[:5].tobytes()
    rs = ix2.rowset()
    t.set_row_base(10)  # the table changes: the index is stale
    for call in (lambda: ix2.find(db[:5]), lambda: ix2.find_db(t), lambda: ix2.rowset()):
        with pytest.raises(capi.GsimError) as e:
            call()
        assert e.value.code == STATE and "changed after the row hash was made" in str(e.value)
    assert ix2.groups()[0].tobytes() == f1.tobytes(), "what the index holds stays readable"
    t.set_row_base(0)
    ix2.close()
    ix2.close()  # (closing twice is harmless)
    assert rs.count == a["groups"], "the row set is independent of the index"
    rs.close()
    t.close()
    e = capi.Table(64).add_rows(np.zeros((0, 2), np.uint32)).finalize(0, 1)
    with e.rowhash() as eix:
        st = eix.stats()
        assert all(st[k] == 0 for k in ("rows", "groups", "repeated_groups", "largest_group", "slots", "launches"))
        f, s = eix.groups()
        assert len(f) == 0 and len(s) == 0
        row, sz = eix.find(np.ones((2, 2), np.uint32))
        assert row.tolist() == [R.ROW_NONE] * 2 and sz.tolist() == [0, 0]
    e.close()
