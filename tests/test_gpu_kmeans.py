"""Lloyd's iteration on the GPU (gsim_db_kmeans) against the rule of tests/kmeans_rule.py: the oracle's scores, numpy's arg-max,
counts and majority votes.  Every comparison is exact.

Planted data: N = 4000 rows at 1024 and 160 bits, six random prototypes of popcount 48, every row a prototype with 4 random bits
flipped (rows of one cluster share at least 40 of about 52 bits, rows of two clusters a handful); init = one row of each cluster.
The planted partition is asserted on the RULE's output before the library is compared with it."""
import numpy as np
import pytest

import kmeans_rule as R
import oracle_lib as O
from gpusimilarity_amd import capi

pytestmark = pytest.mark.gpu
F = np.float32
N, K = 4000, 6

_planted = {}


def planted(bits):
    """-> (rows, cluster of every row, prototypes, init); made once per width, never modified"""
    if bits not in _planted:
        rng = np.random.default_rng(bits)
        proto = np.zeros((K, bits), np.uint8)
        for p in proto:
            p[rng.choice(bits, 48, replace=False)] = 1
        cluster = rng.integers(0, K, N)
        cluster[:K] = np.arange(K)  # (row c is of cluster c: the init)
        B = proto[cluster].copy()
        for row in B:
            row[rng.choice(bits, 4, replace=False)] ^= 1
        pack = lambda b: np.ascontiguousarray(np.packbits(b, axis=1, bitorder="little").view("<u4").astype(np.uint32))
        db, pr = pack(B), pack(proto)
        init = db[:K].copy()
        for a in (db, pr, init, cluster):
            a.setflags(write=False)
        _planted[bits] = (db, cluster, pr, init)
    return _planted[bits]


def table(db):
    return capi.Table(db.shape[1] * 32).add_rows(db).finalize(0, 1)


def same(got, want, what):
    centres, label, score, sizes, st = got
    assert centres.dtype == np.uint32 and label.dtype == np.uint32 and score.dtype == F and sizes.dtype == np.uint32
    assert np.array_equal(centres, want["centres"]), (what, "centres")
    assert np.array_equal(label, want["label"]), (what, "label", int((label != want["label"]).sum()))
    assert np.array_equal(score.view(np.uint32), want["score"].view(np.uint32)), (what, "score")
    assert np.array_equal(sizes, want["sizes"]), (what, "sizes")
    assert st["iterations"] == want["iterations"] and st["converged"] == want["converged"], (what, st, want["iterations"], want["converged"])


@pytest.mark.parametrize("bits", [1024, 160])
def test_the_planted_partition_is_recovered_as_the_rule_says(bits):
    db, cluster, proto, init = planted(bits)
    want = R.kmeans(db, init, 20)
    assert np.array_equal(want["label"], cluster) and want["converged"] == 1 and 2 <= want["iterations"] <= 4, "the rule recovers the planted partition"
    assert np.array_equal(want["centres"], proto), "the majority votes are the prototypes"
    assert np.array_equal(want["sizes"], np.bincount(cluster, minlength=K))
    t = table(db)
    got = t.kmeans(init, 20)
    same(got, want, bits)
    st = got[4]
    assert st["changed_last"] == 0 and st["assign_ms"] > 0 and st["counts_ms"] > 0 and st["wall_ms"] > 0, st
    lab, sc = t.assign(got[0])
    assert np.array_equal(lab, got[1]) and np.array_equal(sc.view(np.uint32), got[2].view(np.uint32)), "assign(centres) reproduces label and score"
    # max_iter = 1: init and its assignment, not converged
    one = t.kmeans(init, 1)
    w1 = R.kmeans(db, init, 1)
    assert w1["iterations"] == 1 and w1["converged"] == 0 and np.array_equal(w1["centres"], init)
    same(one, w1, (bits, "max_iter = 1"))
    assert one[4]["changed_last"] == N
    lab, sc = t.assign(init)
    assert np.array_equal(lab, one[1]) and np.array_equal(sc.view(np.uint32), one[2].view(np.uint32))
    # stopped by max_iter before the labels repeat
    two = t.kmeans(init, 2)
    same(two, R.kmeans(db, init, 2), (bits, "max_iter = 2"))
    t.close()


def test_a_duplicated_centre_stays_empty_and_keeps_its_place():
    """Centres 2 and 6 both start as prototype 2 (no row equals it: every row has 4 bits flipped).  The tie goes to centre 2 in every
    iteration; centre 2's majority vote is the prototype again, so the copy never wins a row and, empty, keeps its centre."""
    db, cluster, proto, init = planted(1024)
    start = np.concatenate([init, proto[2:3]])
    start[2] = proto[2]
    want = R.kmeans(db, start, 20)
    assert want["sizes"][6] == 0 and (want["label"] != 6).all() and np.array_equal(want["centres"][6], proto[2]), "on the rule's output"
    assert np.array_equal(want["label"], cluster) and want["converged"] == 1
    t = table(db)
    got = t.kmeans(start, 20)
    same(got, want, "a duplicated centre")
    assert got[3][6] == 0 and np.array_equal(got[0][6], start[6])
    t.close()


def test_morgan_rows_iteration_for_iteration():
    """m = 50 centres on a Morgan-kind table: the run stopped after 1 ... 5 assignments equals the rule's state at that iteration."""
    n, W, m = 4000, 32, 50
    db = O.synth_rows(41, O.KIND_MORGAN, 0, n, W)
    init = np.ascontiguousarray(db[::80][:m])
    want = R.kmeans(db, init, 5)
    hist = want["history"]
    assert len(hist) >= 3 and not np.array_equal(hist[0][1], hist[1][1]) and not np.array_equal(hist[0][0], hist[1][0]), "the centres and labels move"
    t = table(db)
    for k in range(1, 6):
        centres, label, score, sizes, st = t.kmeans(init, k)
        c_t, l_t = hist[min(k, len(hist)) - 1]
        assert np.array_equal(centres, c_t) and np.array_equal(label, l_t), k
        assert np.array_equal(sizes, np.bincount(l_t, minlength=m)) and st["iterations"] == min(k, len(hist)), (k, st)
    same(t.kmeans(init, 5), want, "max_iter = 5")
    tv = R.tv(0.3, 0.7)
    same(t.kmeans(init, 3, **tv), R.kmeans(db, init, 3, tv), "Tversky (0.3, 0.7)")
    t.close()


def test_an_attached_table_and_the_search_state():
    import torch
    db, cluster, proto, init = planted(160)
    want = R.kmeans(db, init, 20)
    ten = torch.from_numpy(db.view(np.int32).copy()).to("cuda:0")
    a = capi.Table(160)
    a.attach_device_rows(ten.data_ptr(), N, 0)
    same(a.kmeans(init, 20), want, "attached")
    a.close()
    del ten
    t = table(db)
    t.enable_timing(True)
    q = np.ascontiguousarray(db[[7, 1500, 3999]])

    def searches():
        hits, approx = t.search(q, 50, 0.4)
        return b"".join(h.tobytes() for h in hits) + approx.tobytes()

    before = searches()
    counters = ("queries", "handed_back", "rerun_own", "rerun_publish", "rerun_behind", "rerun_torn", "lane_queries", "backoff_skips")
    t0 = t.timing()
    same(t.kmeans(init, 20), want, "between two searches")
    t1 = t.timing()
    assert [t0[c] for c in counters] == [t1[c] for c in counters]
    assert searches() == before
    t.close()
