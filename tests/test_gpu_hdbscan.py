"""HDBSCAN on the GPU: gsim_db_core_scores, gsim_db_mreach_mst and gsim_db_hdbscan.

Expected values: the oracle gives the pair scores (test_gpu_components.score_matrix) and the rule of include/gpusim_hip.h, restated in
hdbscan_rule.py, is applied to them: core scores, the mutual-reachability forest by Kruskal in order E, the multiway condensed tree
with stabilities as fractions, the selection.  Core scores, edges, labels, leave levels, first rows, sizes and birth levels are compared
byte for byte, stabilities to 1e-12 relative (the library sums a few hundred non-negative doubles per cluster; the rule is exact).

Every table is 1000 rows: three full owner tiles of 256 rows and a partial one.  The FAMILY TABLE of a width (`family_table`): 14
families of 120 ... 3 rows, each a sparse centre of 40 bits with a fixed number of bits flipped per member -- 1 in the largest family,
12 in the smallest, so that the families differ in tightness --, 480 KIND_SPARSE background rows, 4 all-zero rows and 4 copies of one
row, shuffled.  test_gpu_components.planted_table is used too, for the forest only.

Non-vacuity, asserted on the EXPECTED result, not on the device's (`not_vacuous`): at (cutoff 0.3, min_pts 5, min_cluster_size 5) on
every width at least 8 selected clusters, at least 100 noise rows and at least 300 edges that share their score with another edge;
every excess-of-mass comparison of a compared case has a relative margin of at least 1e-6, so none hangs on the rounding of a double.
At the smallest cutoff the 128- and 160-bit tables are one tree of 996 rows (sparse rows that narrow pair up by themselves): they are
compared there too.  (The feature request's prototype saw that tree select its single root; with this generator it does not -- 17 and
15 clusters.  What NO_ROOTS changes is asserted at (0.3, min_pts 2, min_cluster_size 3) instead, where from 160 bits on some root
outlives its children, and only-leaves gives more clusters than excess of mass on every width.)"""
import numpy as np
import pytest

import oracle_lib as O
from gpusimilarity_amd import capi
from hdbscan_rule import EOM, LEAF, NO_ROOTS, NOISE, hdbscan_rule, mreach_matrix, tied
from mst_rule import boruvka, mst_rule
from test_gpu_components import LEVELS, TV, knobs, planted_table, score_matrix

pytestmark = pytest.mark.gpu
TINY = float(np.nextafter(np.float32(0), np.float32(1)))
CUTOFFS = (TINY, 0.3)
MIN_PTS = (1, 2, 5, 16)
WIDTHS = [128, 160, 512, 1024, 2048, 4096]
N = 1000
FAMILIES = (120, 90, 70, 55, 45, 35, 28, 22, 16, 12, 8, 5, 3, 3)
_TABLES, _WANT, _SELECTED = {}, {}, {}


def table(db, mst_pairs=None, knn_pairs=None, base=0):
    with knobs(GSIM_MST_LAUNCH_PAIRS=mst_pairs, GSIM_KNN_LAUNCH_PAIRS=knn_pairs):
        t = capi.Table(db.shape[1] * 32).add_rows(db).finalize(0, 1)
    if base:
        t.set_row_base(base)
    return t


def flip(row, bits):
    for bit in bits:
        row[bit // 32] ^= np.uint32(1 << (bit % 32))


def family_table(bits):
    """(rows, the oracle's Tanimoto scores) of the family table of that width: made once, never changed"""
    if bits not in _TABLES:
        W = bits // 32
        rng = np.random.default_rng(1)
        rows = []
        for k, members in enumerate(FAMILIES):
            centre = np.zeros(W, np.uint32)
            flip(centre, rng.choice(bits, 40, replace=False))
            flips = 1 + k * 11 // (len(FAMILIES) - 1)
            for _ in range(members):
                row = centre.copy()
                flip(row, rng.choice(bits, flips, replace=False))
                rows.append(row)
        background = O.synth_rows(0x4DB5 + bits, O.KIND_SPARSE, 0, N - len(rows) - 8, W)
        db = np.concatenate([np.stack(rows), background, np.zeros((4, W), np.uint32), np.repeat(background[:1], 4, 0)])
        assert len(db) == N and background[0].any()
        db = np.ascontiguousarray(db[rng.permutation(N)])
        S = score_matrix(db)
        for x in (db, S):
            x.setflags(write=False)
        _TABLES[bits] = (db, S)
    return _TABLES[bits]


def expected(name, S, cutoff, min_pts):
    """(edges by Kruskal on m, rounds, owners per scan, core, m) -- made once; Boruvka on m must build the very same forest"""
    key = (name, cutoff, min_pts)
    if key not in _WANT:
        M, core = mreach_matrix(S, cutoff, min_pts)
        edges = mst_rule(M, cutoff)
        by_rounds, rounds, scans = boruvka(M, cutoff)
        assert by_rounds.tobytes() == edges.tobytes(), key
        for x in (edges, core, M):
            x.setflags(write=False)
        _WANT[key] = (edges, rounds, scans, core, M)
    return _WANT[key]


def selection(name, S, cutoff, min_pts, mcs, flags):
    key = (name, cutoff, min_pts, mcs, flags)
    if key not in _SELECTED:
        _SELECTED[key] = hdbscan_rule(expected(name, S, cutoff, min_pts)[0], len(S), cutoff, mcs, flags)
    return _SELECTED[key]


def not_vacuous(bits):
    S = family_table(bits)[1]
    rule = selection(bits, S, 0.3, 5, 5, EOM)
    return (len(rule["sizes"]), int((rule["label"] == NOISE).sum()), tied(expected(bits, S, 0.3, 5)[0]),
            min(rule["margins"]) if rule["margins"] else 1.0)


def same_forest(got, want, what, base=0):
    edges, core, st = got
    w = want[0].copy()
    w["a"] += np.uint32(base)
    w["b"] += np.uint32(base)
    assert core.tobytes() == want[3].tobytes(), (what, core[:8], want[3][:8])
    assert len(edges) == len(w) and st["edges"] == len(w), (what, len(edges), len(w), st)
    assert edges.tobytes() == w.tobytes(), (what, edges[:8], w[:8])
    n = st["rows"]
    assert st["rounds"] == want[1] and st["scan_owners"] == want[2] and st["scans"] == len(want[2]), (what, st, want[1:3])
    assert st["owner_rows"] == sum(want[2][:want[1]]) and st["pairs"] == sum(want[2]) * n, (what, st)
    with np.errstate(invalid="ignore"):
        assert st["core_rows"] == int((want[3] >= np.float32(what[1])).sum()), (what, st)


def same_selection(got, want, what, base=0):
    label, leave, first_row, sizes, birth, stability = got[:6]
    assert label.tobytes() == want["label"].tobytes(), (what, label[:20], want["label"][:20])
    assert leave.tobytes() == want["leave"].tobytes(), (what, leave[:20], want["leave"][:20])
    assert first_row.tobytes() == (want["first_row"] + np.uint32(base)).tobytes() and sizes.tobytes() == want["sizes"].tobytes(), what
    assert birth.tobytes() == want["birth"].tobytes(), (what, birth, want["birth"])
    assert len(stability) == len(want["stability"])
    for x, y in zip(stability.tolist(), want["stability"]):
        assert abs(x - float(y)) <= 1e-12 * float(y), (what, x, y)


def dbscan_star(t, edges, core, cutoff, min_pts, what):
    """consequence 2: at every level >= cutoff, the cut of the forest restricted to the rows with core >= level is DBSCAN's partition
    of its core rows, and every other row is a singleton of the cut"""
    for level in (c for c in LEVELS if c >= cutoff):
        comp, _, sizes = capi.mst_cut(edges, N, level)
        label, degree, _, _, _, _ = t.dbscan(level, min_pts)
        dense = degree + 1 >= min_pts
        assert np.array_equal(dense, core >= np.float32(level)), (what, level)
        assert (sizes[comp[~dense]] == 1).all(), (what, level, "a row that is not dense is a singleton")
        pairs = set(zip(comp[dense].tolist(), label[dense].tolist()))
        assert len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs}), (what, level, "the same partition of the cores")
        assert NOISE not in {p[1] for p in pairs}


@pytest.mark.parametrize("bits", WIDTHS)
def test_parity_with_the_rule(bits):
    """160 bits takes the zero-padded copy; the six widths are the six instantiations of the fold kernel"""
    db, S = family_table(bits)
    clusters, noise, ties, margin = not_vacuous(bits)
    assert clusters >= 8 and noise >= 100 and ties >= 300 and margin >= 1e-6, (bits, clusters, noise, ties, margin)
    t = table(db)
    plain = {cutoff: t.mst(cutoff) for cutoff in CUTOFFS}
    for cutoff in CUTOFFS:
        graph = t.neighbors(cutoff)
        for min_pts in MIN_PTS:
            what = (bits, cutoff, min_pts)
            want = expected(bits, S, cutoff, min_pts)
            got = t.mreach_mst(min_pts, cutoff)
            same_forest(got, want, what)
            again = t.mreach_mst(min_pts, cutoff)
            assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes(), "two runs give identical bytes"
            assert (again[2]["rounds"], again[2]["scan_owners"]) == (got[2]["rounds"], got[2]["scan_owners"])
            if min_pts == 1:
                assert got[0].tobytes() == plain[cutoff][0].tobytes(), (what, "min_pts 1 is gsim_db_mst")
                assert (got[2]["rounds"], got[2]["scan_owners"]) == (plain[cutoff][1]["rounds"], plain[cutoff][1]["scan_owners"])
                assert got[2]["core_launches"] == 0 and got[2]["core_rows"] == N
            else:
                # with min_pts 2 a row's core score is its best neighbour's: it caps nothing, and rows without a neighbour have no edge
                # anyway; beyond that the core scores must cap something
                assert (got[0].tobytes() == plain[cutoff][0].tobytes()) == (min_pts == 2), (what, "what the core scores cap")
                # core scores on their own: the last entries of the k-nearest-neighbour lists
                core, cst = t.core_scores(min_pts, cutoff)
                indptr, _, scores = t.knn(min_pts - 1, cutoff)
                full = np.diff(indptr.astype(np.int64)) == min_pts - 1
                last = np.where(full, scores[np.where(full, indptr[1:].astype(np.int64) - 1, 0)], np.float32(0)).astype(np.float32)
                assert core.tobytes() == last.tobytes() == got[1].tobytes(), what
                assert cst["entries"] == int(full.sum()) == got[2]["core_rows"] and cst["launches"] == got[2]["core_launches"] == 1, (what, cst)
            dbscan_star(t, got[0], got[1], cutoff, min_pts, what)
            # consequence 3: the same forest from the neighbour lists and the host function
            by_host = capi.mreach_mst(*graph, min_pts)
            assert by_host[0].tobytes() == got[0].tobytes() and by_host[1].tobytes() == got[1].tobytes(), what
    t.close()


@pytest.mark.parametrize("bits", [160, 1024])
def test_the_planted_tables_give_the_rules_forest(bits):
    """test_gpu_mst's tables: a block of 600 identical rows (core 1.0 for every min_pts here), chains, duplicates"""
    db, _, S = planted_table(bits)
    t = table(db)
    for cutoff, min_pts in ((TINY, 5), (0.5, 2), (0.5, 16), (0.7, 5)):
        want = expected(("planted", bits), S, cutoff, min_pts)
        assert tied(want[0]) >= 599 and want[1] >= (2 if min_pts == 2 or cutoff == TINY else 1), (bits, cutoff, min_pts, want[1], tied(want[0]))
        same_forest(t.mreach_mst(min_pts, cutoff), want, (bits, cutoff, min_pts))
    t.close()


@pytest.mark.parametrize("bits", WIDTHS)
def test_hdbscan_equals_the_rule(bits):
    db, S = family_table(bits)
    t = table(db)
    cases = [(0.3, 5, 5), (0.3, 2, 3), (0.3, 16, 10)] + ([(TINY, 5, 5)] if bits <= 160 else [])
    for cutoff, min_pts, mcs in cases:
        edges = t.mreach_mst(min_pts, cutoff)[0]
        for flags in (EOM, LEAF, EOM | NO_ROOTS):
            what = (bits, cutoff, min_pts, mcs, flags)
            want = selection(bits, S, cutoff, min_pts, mcs, flags)
            assert not want["margins"] or min(want["margins"]) >= 1e-6, (what, min(want["margins"]))
            got = t.hdbscan(min_pts, mcs, cutoff, flags=flags)
            same_selection(got, want, what)
            st = got[6]
            assert st["clusters"] == len(want["sizes"]) and st["noise"] == int((want["label"] == NOISE).sum()) and st["edges"] == len(edges), st
            by_host = capi.mst_hdbscan(edges, N, cutoff, mcs, flags)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(by_host, got[:6])), (what, "the two steps on their own")
        if (cutoff, min_pts, mcs) == (0.3, 2, 3) and bits >= 160:  # trees whose root outlives its children: NO_ROOTS tells them apart
            root, split = selection(bits, S, cutoff, min_pts, mcs, EOM), selection(bits, S, cutoff, min_pts, mcs, EOM | NO_ROOTS)
            assert len(split["sizes"]) > len(root["sizes"]) >= 8, (bits, len(root["sizes"]), len(split["sizes"]))
        if (cutoff, min_pts, mcs) == (0.3, 2, 3):  # and only leaves is yet another answer
            assert len(selection(bits, S, cutoff, min_pts, mcs, LEAF)["sizes"]) > len(selection(bits, S, cutoff, min_pts, mcs, EOM)["sizes"])
    t.close()


@pytest.mark.parametrize("bits", [160, 1024])
def test_passes_cut_into_many_launches_give_the_same_bytes(bits):
    db, S = family_table(bits)
    # one column tile of 256 candidates per launch: 4 launches per scan and 4 for the core pass
    whole, cut = table(db), table(db, mst_pairs=1, knn_pairs=1)
    for cutoff, min_pts in ((TINY, 5), (0.3, 16)):
        want = expected(bits, S, cutoff, min_pts)
        a, b = whole.mreach_mst(min_pts, cutoff), cut.mreach_mst(min_pts, cutoff)
        sa, sb = a[2], b[2]
        assert sa["launches"] == sa["scans"] and sb["launches"] == 4 * sb["scans"] and sb["scans"] == sa["scans"] >= 2, (sa, sb)
        assert sa["core_launches"] == 1 and sb["core_launches"] == 4
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (bits, cutoff, min_pts)
        same_forest(b, want, (bits, cutoff, min_pts))
        assert cut.core_scores(min_pts, cutoff)[0].tobytes() == want[3].tobytes()
        got = cut.hdbscan(min_pts, 5, cutoff)
        same_selection(got, selection(bits, S, cutoff, min_pts, 5, EOM), ("cut", bits, cutoff, min_pts))
    whole.close()
    cut.close()


def test_row_base_and_the_search_state():
    base, cutoff, min_pts = 7000, 0.3, 5
    db, S = family_table(2048)
    want = expected(2048, S, cutoff, min_pts)
    rule = selection(2048, S, cutoff, min_pts, 5, EOM)
    t = table(db)
    singles = np.ascontiguousarray(db[[3, 500, N - 1]])

    def searches():
        hits, approx = t.search(singles, 50)
        return b"".join(h.tobytes() for h in hits) + approx.tobytes()

    before = searches()
    same_forest(t.mreach_mst(min_pts, cutoff), want, (2048, cutoff, min_pts))
    same_selection(t.hdbscan(min_pts, 5, cutoff), rule, "no base")
    assert t.core_scores(min_pts, cutoff)[0].tobytes() == want[3].tobytes()
    assert searches() == before, "the search state is as it was"
    for failing in (lambda: t.mreach_mst(min_pts, 1.5), lambda: t.hdbscan(0, 5, cutoff), lambda: t.core_scores(130, cutoff)):
        with pytest.raises(capi.GsimError):
            failing()  # a failed call ...
    assert searches() == before
    t.set_row_base(base)  # ... and correct ones right after it: the base goes to the edges and to first_row, not to the labels
    same_forest(t.mreach_mst(min_pts, cutoff), want, (2048, cutoff, min_pts), base=base)
    same_selection(t.hdbscan(min_pts, 5, cutoff), rule, "row base", base=base)
    t.close()


def test_tversky():
    db, _ = family_table(1024)
    S = score_matrix(db, TV)
    t = table(db)
    want = expected(("tversky", 1024), S, 0.3, 5)
    assert tied(want[0]) >= 300 and want[0].tobytes() != expected(1024, family_table(1024)[1], 0.3, 5)[0].tobytes(), "Dice is not Tanimoto"
    same_forest(t.mreach_mst(5, 0.3, **TV), want, (1024, 0.3, 5))
    rule = hdbscan_rule(want[0], N, 0.3, 5, EOM)
    assert len(rule["sizes"]) >= 8 and all(m >= 1e-6 for m in rule["margins"])
    same_selection(t.hdbscan(5, 5, 0.3, **TV), rule, "tversky")
    t.close()


def test_edges():
    db, S = family_table(1024)
    # min_pts beyond the table: no row is dense
    small = np.ascontiguousarray(db[:40])
    t = table(small)
    for min_pts in (41, 42, 129):
        edges, core, st = t.mreach_mst(min_pts, TINY)
        assert len(edges) == 0 and not core.any() and st["core_rows"] == 0 and st["rounds"] == 0 and st["scan_owners"] == [40], (min_pts, st)
        out = t.hdbscan(min_pts, 2, TINY)
        assert (out[0] == NOISE).all() and not out[1].any() and len(out[2]) == 0 and out[6]["noise"] == 40
    t.close()
    # four duplicates and three all-zero rows among unrelated rows: at min_pts 4 the duplicates are each other's three neighbours
    row = np.zeros(32, np.uint32)
    flip(row, range(100, 130))
    other = np.zeros((5, 32), np.uint32)
    for k in range(5):
        flip(other[k], range(200 + 40 * k, 230 + 40 * k))
    mixed = np.stack([other[0], row, np.zeros(32, np.uint32), row, other[1], np.zeros(32, np.uint32), row, other[2], row, other[3],
                      np.zeros(32, np.uint32), other[4]])
    t = table(mixed)
    edges, core, st = t.mreach_mst(4, TINY)
    assert core.tolist() == [0, 1, 0, 1, 0, 0, 1, 0, 1, 0, 0, 0] and edges.tolist() == [(1, 3, 1.0), (1, 6, 1.0), (1, 8, 1.0)] and st["core_rows"] == 4
    label, leave, first, sizes, birth, stab, _ = t.hdbscan(4, 4, 0.5)
    assert label.tolist() == [NOISE, 0, NOISE, 0, NOISE, NOISE, 0, NOISE, 0, NOISE, NOISE, NOISE] and sizes.tolist() == [4] and stab.tolist() == [2.0]
    assert birth.tolist() == [0.5] and first.tolist() == [1] and leave[[1, 3, 6, 8]].tolist() == [1.0] * 4
    # all-zero rows are isolated even at min_pts 1, where their core score is 1.0
    edges, core, _ = t.mreach_mst(1, TINY)
    assert core.tolist() == [1.0] * 12 and not (set(edges["a"].tolist()) | set(edges["b"].tolist())) & {2, 5, 10}
    assert edges.tobytes() == t.mst(TINY)[0].tobytes()
    t.close()
    # no row, one row, two rows
    empty = capi.Table(1024)
    assert len(empty.mreach_mst(5, 0.5)[0]) == 0 and len(empty.core_scores(5, 0.5)[0]) == 0 and len(empty.hdbscan(5, 5, 0.5)[0]) == 0
    t = table(mixed[1:2])
    edges, core, st = t.mreach_mst(2, 0.5)
    assert len(edges) == 0 and core.tolist() == [0.0] and st["rows"] == 1 and st["scans"] == st["core_launches"] == 0
    assert t.mreach_mst(1, 0.5)[1].tolist() == [1.0] and t.core_scores(1, 0.5)[0].tolist() == [1.0] and t.core_scores(2, 0.5)[0].tolist() == [0.0]
    assert t.hdbscan(1, 2, 0.5)[0].tolist() == [NOISE]
    t.close()
    t = table(np.ascontiguousarray(mixed[[1, 3]]))
    edges, core, st = t.mreach_mst(2, 1.0)
    assert edges.tolist() == [(0, 1, 1.0)] and core.tolist() == [1.0, 1.0] and st["rounds"] == st["scans"] == 1
    assert len(t.mreach_mst(3, 1.0)[0]) == 0
    label, _, first, sizes, birth, stab, _ = t.hdbscan(2, 2, 0.5)
    assert label.tolist() == [0, 0] and (first.tolist(), sizes.tolist(), birth.tolist(), stab.tolist()) == ([0], [2], [0.5], [1.0])
    t.close()


def test_generated_and_attached_tables():
    """no host copy exists: the expected rows are regenerated with gsim_synth_row; 160 bits attached: a zero-padded copy"""
    import torch
    n, bits, seed = 1000, 1024, 0xC0119
    rows = np.stack([capi.synth_row(seed, O.KIND_MORGAN, r, bits) for r in range(n)])
    S = score_matrix(rows)
    want = expected(("generated", bits), S, 0.3, 3)
    rule = hdbscan_rule(want[0], n, 0.3, 3, EOM)
    assert 400 <= len(want[0]) < n - 1 and want[1] >= 2 and len(rule["sizes"]) >= 4 and all(m >= 1e-6 for m in rule["margins"])
    g = capi.Table(bits).generate(seed, O.KIND_MORGAN, 0, n, 0)
    same_forest(g.mreach_mst(3, 0.3), want, (bits, 0.3, 3))
    same_selection(g.hdbscan(3, 3, 0.3), rule, "generated")
    g.close()
    narrow, S = family_table(160)
    ten = torch.from_numpy(narrow.view(np.int32).copy()).to("cuda:0")
    a = capi.Table(160)
    a.attach_device_rows(ten.data_ptr(), len(narrow), 0)
    same_forest(a.mreach_mst(5, 0.3), expected(160, S, 0.3, 5), (160, 0.3, 5))
    same_selection(a.hdbscan(5, 5, 0.3), selection(160, S, 0.3, 5, 5, EOM), "attached")
    a.close()
