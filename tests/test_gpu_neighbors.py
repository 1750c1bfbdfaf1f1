"""gsim_db_neighbors on the GPU: every row's list against the oracle (indices exactly, scores bit for bit), the edge cases
of the CSR build and the launch schedule, and consistency with gsim_db_search on a 1 M-row table."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from gpusimilarity_amd import capi
from gpusimilarity_amd.fingerprintdb import FingerprintDB

pytestmark = pytest.mark.gpu
NT = 16
TV = dict(metric=capi.METRIC_TVERSKY, alpha=0.5, beta=0.5)


def table(db, device=0):
    return capi.Table(db.shape[1] * 32).add_rows(db).finalize(device, 1)


def oracle_lists(db, cutoff, metric=O.METRIC_TANIMOTO, alpha=1.0, beta=1.0, rows=None):
    """row i -> (columns ascending, scores): oracle_lib.search(row i, table, k = N, cutoff) minus row i."""
    n = db.shape[0]
    out = {}
    for i in (range(n) if rows is None else rows):
        hits, _ = O.search(db[i], db, n, cutoff, metric, alpha, beta, nthreads=NT)
        hits = hits[hits["row"] != i]
        o = np.argsort(hits["row"], kind="stable")
        out[i] = (hits["row"][o].astype(np.uint32), hits["score"][o])
    return out


def check_against(csr, want, cutoff, row_begin=0, row_base=0):
    indptr, indices, scores = csr
    for i, (cols, sc) in want.items():
        keep = sc >= np.float32(cutoff)
        lo, hi = int(indptr[i - row_begin]), int(indptr[i - row_begin + 1])
        assert np.array_equal(indices[lo:hi], cols[keep] + np.uint32(row_base)), (i, cutoff)
        assert np.array_equal(scores[lo:hi].view(np.uint32), sc[keep].view(np.uint32)), (i, cutoff)


WIDTHS = [128, 160, 256, 512, 896, 1024, 2048, 4096]
KINDS = [O.KIND_SPARSE, O.KIND_DENSE, O.KIND_MORGAN]


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_oracle(bits, kind):
    W = bits // 32
    n = 1200 if kind != O.KIND_DENSE else 700
    db = O.synth_rows(0xBE11 + bits + 7 * kind, kind, 0, n, W)
    db[n // 3] = db[5]  # duplicates: score 1.0
    db[n // 2] = 0      # an all-zero row: nobody's neighbour
    t = table(db)
    for metric_kw, ocut in ((dict(), 0.3), (TV, 0.5)):
        want = oracle_lists(db, ocut, metric_kw.get("metric", 0), metric_kw.get("alpha", 1.0), metric_kw.get("beta", 1.0))
        for cutoff in (0.3, 0.5, 0.7, 1.0):
            if cutoff < ocut:
                continue
            got = t.neighbors(cutoff, **metric_kw)
            assert len(got[0]) == n + 1 and int(got[0][-1]) == len(got[1])
            check_against(got, want, cutoff)
    assert int(t.neighbors(0.3)[0][n // 2 + 1] - t.neighbors(0.3)[0][n // 2]) == 0
    t.close()


def test_cutoff_equal_to_scores_that_occur():
    """cutoff 0.5 with c / (a + b - c) = 1/2 pairs present: they are listed (>=), and 1/3 ones at cutoff 1/3."""
    n, W = 900, 32
    db = O.synth_rows(0x7133, O.KIND_SPARSE, 0, n, W)

    def bits(*ranges):
        x = np.zeros(W * 32, np.uint8)
        for lo, hi in ranges:
            x[lo:hi] = 1
        return np.packbits(x, bitorder="little").view(np.uint32)

    db[10] = bits((0, 40))             # 40 bits
    db[11] = bits((0, 20))             # vs 10: c = 20, a + b - c = 40: exactly 1/2
    db[12] = bits((0, 10), (40, 50))   # vs 11: c = 10, a + b - c = 30: RN(1/3)
    t = table(db)
    want = oracle_lists(db, 0.3)
    sc_all = np.concatenate([v[1] for v in want.values()])
    for cutoff in (np.float32(0.5), np.float32(1.0) / np.float32(3.0)):
        assert (sc_all == cutoff).any(), cutoff
        check_against(t.neighbors(float(cutoff)), want, float(cutoff))
    t.close()


def test_twenty_thousand_rows():
    n, W = 20000, 32
    db = O.synth_rows(0x20000, O.KIND_MORGAN, 0, n, W)
    t = table(db)
    got5, got7 = t.neighbors(0.5), t.neighbors(0.7)
    want = oracle_lists(db, 0.5)
    check_against(got5, want, 0.5)
    check_against(got7, want, 0.7)
    t.close()


@pytest.mark.skipif(O.ref_lib() is None, reason="oracle/_ref (the reference's own functor) was not built: build() makes it "
                                                 "where the reference sources are present")
def test_reference_functor_pins_the_tanimoto_lists():
    """Every 97th row's list against the reference's own TanimotoFunctorCPU (RefTable.scan) on a 20 000-row table."""
    n, W = 20000, 32
    db = O.synth_rows(0x20000, O.KIND_MORGAN, 0, n, W)
    t = table(db)
    indptr, indices, scores = t.neighbors(0.7)
    t.close()
    ref = O.RefTable(db)
    for i in range(0, n, 97):
        s = ref.scan(db[i], nthreads=NT)
        cols = np.flatnonzero(s >= np.float32(0.7))
        cols = cols[cols != i]
        lo, hi = int(indptr[i]), int(indptr[i + 1])
        assert np.array_equal(indices[lo:hi], cols.astype(np.uint32)), i
        assert np.array_equal(scores[lo:hi].view(np.uint32), s[cols].view(np.uint32)), i
    ref.close()


@pytest.mark.parametrize("bits", [1024, 160])
def test_attached_device_rows(bits):
    """Rows borrowed from a torch tensor (gsim_db_attach_device_rows): at 1024 bits the kernel reads the caller's own
    memory (no padded copy), at 160 bits a zero-padded copy of it; both equal the uploaded table's lists."""
    import torch
    n, W = 2500, bits // 32
    db = O.synth_rows(0xA77 + bits, O.KIND_MORGAN, 0, n, W)
    ten = torch.from_numpy(db.view(np.int32).copy()).to("cuda:0")
    t = capi.Table(bits)
    t.attach_device_rows(ten.data_ptr(), n, 0)
    got = t.neighbors(0.5)
    part = t.neighbors(0.5, row_begin=700, row_end=2222)
    t.close()
    u = table(db)
    want = u.neighbors(0.5)
    u.close()
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(part[1], want[1][int(want[0][700]):int(want[0][2222])])
    check_against(got, oracle_lists(db, 0.5, rows=range(0, n, 11)), 0.5)
    del ten


def test_one_and_two_rows():
    x = O.synth_rows(3, O.KIND_SPARSE, 0, 2, 32)
    t = table(x[:1])
    indptr, indices, scores = t.neighbors(0.5)
    assert list(indptr) == [0, 0] and len(indices) == 0 and len(scores) == 0
    t.close()
    t = table(np.stack([x[0], x[0]]))
    indptr, indices, scores = t.neighbors(1.0)
    assert list(indptr) == [0, 1, 2] and list(indices) == [1, 0] and list(scores) == [1.0, 1.0]
    t.close()
    t = table(x)
    s = O.search(x[0], x, 2, 0.0)[0]
    s01 = s[s["row"] == 1]["score"][0]
    indptr, indices, scores = t.neighbors(float(s01))
    assert list(indptr) == [0, 1, 2] and list(indices) == [1, 0]
    assert scores.view(np.uint32).tolist() == [s01.view(np.uint32)] * 2
    if s01 < 1.0:
        assert list(t.neighbors(float(np.nextafter(s01, np.float32(2))))[0]) == [0, 0, 0]
    t.close()


def test_all_zero_rows():
    db = np.zeros((300, 32), np.uint32)
    db[100:110] = O.synth_rows(9, O.KIND_SPARSE, 0, 1, 32)[0]
    t = table(db)
    for kw in ({}, TV):
        indptr, indices, scores = t.neighbors(0.1, **kw)
        counts = np.diff(indptr.astype(np.int64))
        assert counts[100:110].tolist() == [9] * 10 and counts.sum() == 90
        assert (scores == 1.0).all()
    t.close()


def test_overflow_runs_the_overflowed_launches_once_more():
    """1 500 identical rows list 1500 x 1499 pairs, more than the pair buffer holds on a handle's first call: the launches
    from the first one that overflowed run again (launches_rerun > 0), and the result is complete."""
    n = 1500
    row = O.synth_rows(11, O.KIND_DENSE, 0, 1, 4)[0]
    db = np.tile(row, (n, 1))
    t = table(db)
    st = {}
    indptr, indices, scores = t.neighbors(0.9, stats=st)
    assert st["launches_rerun"] > 0 and st["pairs"] == n * (n - 1) // 2, st
    assert (np.diff(indptr.astype(np.int64)) == n - 1).all()
    for i in (0, 1, 777, n - 1):
        lo, hi = int(indptr[i]), int(indptr[i + 1])
        assert indices[lo:hi].tolist() == [j for j in range(n) if j != i]
    assert (scores == 1.0).all()
    st2 = {}
    again = t.neighbors(0.9, stats=st2)  # the buffer grew: no rerun now, same bytes
    assert st2["launches_rerun"] == 0
    assert all(np.array_equal(a, b) for a, b in zip((indptr, indices, scores), again))
    t.close()


def test_ranges_rows_base_determinism_and_search_state():
    n, W = 3000, 16
    db = O.synth_rows(0xA11, O.KIND_MORGAN, 0, n, W)
    t = table(db)
    q = db[[7, 1500, 2999]]
    before = t.search(q, 50, 0.4)
    full = t.neighbors(0.55)
    again = t.neighbors(0.55)
    for a, b in zip(full, again):
        assert a.tobytes() == b.tobytes()  # byte-identical from run to run
    after = t.search(q, 50, 0.4)
    for h0, h1 in zip(before[0], after[0]):
        assert h0.tobytes() == h1.tobytes()
    assert np.array_equal(before[1], after[1])
    # pieces not aligned to any tile size make up the full call
    cuts = [0, 1, 255, 257, 1000, 1789, 2999, 3000]
    ind, sc = [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        p_indptr, p_ind, p_sc = t.neighbors(0.55, row_begin=lo, row_end=hi)
        assert len(p_indptr) == hi - lo + 1
        assert np.array_equal(p_indptr.astype(np.int64), full[0][lo:hi + 1].astype(np.int64) - int(full[0][lo]))
        ind.append(p_ind)
        sc.append(p_sc)
    assert np.array_equal(np.concatenate(ind), full[1])
    assert np.array_equal(np.concatenate(sc).view(np.uint32), full[2].view(np.uint32))
    empty = t.neighbors(0.55, row_begin=17, row_end=17)
    assert list(empty[0]) == [0] and len(empty[1]) == 0
    # row_base: added to every column index
    t.set_row_base(1_000_000)
    based = t.neighbors(0.55)
    assert np.array_equal(based[0], full[0]) and np.array_equal(based[1], full[1] + np.uint32(1_000_000))
    part = t.neighbors(0.55, row_begin=999, row_end=1234)
    assert np.array_equal(part[1], full[1][int(full[0][999]):int(full[0][1234])] + np.uint32(1_000_000))
    t.close()
    want = oracle_lists(db, 0.55, rows=range(0, n, 37))
    check_against(full, want, 0.55)


def test_error_codes_on_the_gpu():
    db = O.synth_rows(5, O.KIND_SPARSE, 0, 512, 32)
    t = table(db)
    for bad in (0.0, -1.0, 1.01):
        with pytest.raises(capi.GsimError) as e:
            t.neighbors(bad)
        assert e.value.code == -1
    with pytest.raises(capi.GsimError) as e:
        t.neighbors(0.5, metric=capi.METRIC_TVERSKY, alpha=0.3, beta=0.7)
    assert e.value.code == -1
    t.close()
    f = capi.Table(1024).add_rows(db).set_fold_factor(2).finalize(0, 1)
    with pytest.raises(capi.GsimError) as e:
        f.neighbors(0.5)
    assert e.value.code == -5
    f.close()
    # a multi-shard handle: two logical devices on one GPU (the test-hooks build of the library)
    from conftest import hooks_env, HOOKS_LIB
    assert os.path.exists(HOOKS_LIB)
    code = ("import sys; sys.path.insert(0, %r); import numpy as np; from gpusimilarity_amd import capi\n"
            "t = capi.Table(1024).add_rows(np.ones((512, 32), np.uint32)).finalize(0, 2)\n"
            "assert t.shard_count() == 2\n"
            "try:\n    t.neighbors(0.5)\nexcept capi.GsimError as e:\n    print('code', e.code)\n"
            % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r = subprocess.run([sys.executable, "-c", code], env=hooks_env(GSIM_TEST_ALIAS_DEVICES="2"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "code -5" in r.stdout, r.stdout + r.stderr


def test_generated_table_and_fingerprintdb_butina():
    n, W = 5000, 32
    t = capi.Table(1024).generate(0x5EED, capi.SYNTH_MORGAN, 0, n, 0)
    db = O.synth_rows(0x5EED, O.KIND_MORGAN, 0, n, W)
    got = t.neighbors(0.6)
    t.close()
    check_against(got, oracle_lists(db, 0.6, rows=range(0, n, 23)), 0.6)
    fdb = FingerprintDB(1024, n, "k", [db], [b"s%d" % i for i in range(n)], [b"i%d" % i for i in range(n)])
    fdb.copyToGPU()
    indptr, indices, scores = fdb.neighbors(0.6)
    assert np.array_equal(indptr, got[0]) and np.array_equal(indices, got[1])
    clusters = fdb.butina(0.6)
    # the stated rule, restated
    order = sorted(range(n), key=lambda r: (int(indptr[r + 1] - indptr[r]), r), reverse=True)
    seen = np.zeros(n, bool)
    want = []
    for r in order:
        if seen[r]:
            continue
        nb = [int(j) for j in indices[indptr[r]:indptr[r + 1]] if not seen[j]]
        seen[r] = True
        seen[nb] = True
        want.append((r,) + tuple(sorted(nb)))
    assert clusters == want
    assert sorted(x for c in clusters for x in c) == list(range(n))


def test_consistency_with_search_at_one_million_rows():
    n, W, cutoff = 1_000_000, 32, 0.7
    t = capi.Table(1024).generate(0xC0FFEE, capi.SYNTH_MORGAN, 0, n, 0)
    indptr, indices, scores = t.neighbors(cutoff)
    rng = np.random.default_rng(1)
    rows = np.sort(rng.choice(n, 2000, replace=False))
    q = np.stack([capi.synth_row(0xC0FFEE, capi.SYNTH_MORGAN, int(r), 1024) for r in rows])
    hits, approx = t.search(q, 100, cutoff)
    checked = 0
    for qi, r in enumerate(rows):
        lo, hi = int(indptr[r]), int(indptr[r + 1])
        if q[qi].any():
            assert hi - lo == int(approx[qi]) - 1, (r, hi - lo, int(approx[qi]))
            checked += 1
        cols, sc = indices[lo:hi], scores[lo:hi]
        o = np.lexsort((cols, -sc.astype(np.float64)))
        h = hits[qi][hits[qi]["row"] != r]
        assert np.array_equal(cols[o][:len(h)], h["row"]), r
        assert np.array_equal(sc[o][:len(h)].view(np.uint32), h["score"].view(np.uint32)), r
    assert checked > 1900
    t.close()
