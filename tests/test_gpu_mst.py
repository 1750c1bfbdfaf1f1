"""Exact single-linkage dendrograms on the GPU (gsim_db_mst).

Expected values: the oracle gives the pair scores (test_gpu_components.score_matrix, on its planted 1000-row tables) and the rule of
include/gpusim_hip.h, restated in mst_rule.py as Kruskal in order E, is applied to them.  Every comparison is exact: the edges byte for
byte, and their count.

Non-vacuity (`not_vacuous`), asserted on the EXPECTED result: at the four loosest cutoffs the reference Boruvka of mst_rule.py takes at
least 3 rounds on the tables of 512 bits and more (the 128- and 160-bit tables: at the two loosest; 2 rounds at 0.5 and 0.7), exactly 1
round at cutoff 1.0; at least 600 of the expected edges share their score with another edge; at 0.5 the forest has at least 5 trees of
more than one row and fewer than N - 1 edges.  The device's round count and the owner count of every scan must equal the rule's."""
import numpy as np
import pytest

import oracle_lib as O
from gpusimilarity_amd import capi
from mst_rule import boruvka, mst_rule
from test_gpu_components import LEVELS, TV, knobs, planted_table, score_matrix

pytestmark = pytest.mark.gpu
PAIRS = "GSIM_MST_LAUNCH_PAIRS"
TINY = float(np.nextafter(np.float32(0), np.float32(1)))
CUTOFFS = (TINY, 0.15, 0.5, 0.7, 1.0)
N = 1000
_WANT = {}


def table(db, pairs=None, base=0):
    with knobs(**{PAIRS: pairs}):
        t = capi.Table(db.shape[1] * 32).add_rows(db).finalize(0, 1)
    if base:
        t.set_row_base(base)
    return t


def expected(bits, cutoff, kw=None, S=None):
    """(edges by Kruskal, rounds, owners per scan) of a planted table: made once; Boruvka must build the very same forest"""
    key = (bits, cutoff, bool(kw))
    if key not in _WANT:
        S = planted_table(bits)[2] if S is None else S
        edges = mst_rule(S, cutoff)
        by_rounds, rounds, scans = boruvka(S, cutoff)
        assert by_rounds.tobytes() == edges.tobytes(), key
        edges.setflags(write=False)
        _WANT[key] = (edges, rounds, scans)
    return _WANT[key]


def tied(edges):
    _, counts = np.unique(edges["score"], return_counts=True)
    return int(counts[counts > 1].sum())


def not_vacuous(bits, cutoff, want):
    edges, rounds, _ = want
    comp, _, sizes = capi.mst_cut(edges, N, 0.0)
    if cutoff == 1.0:
        ok = rounds == 1
    elif bits >= 512 or cutoff < 0.5:
        ok = rounds >= 3
    else:
        ok = rounds == 2
    if cutoff == 0.5:
        ok = ok and int((sizes > 1).sum()) >= 5 and len(edges) < N - 1
    return ok and tied(edges) >= 600


def same(got, want, what, base=0):
    edges, st = got
    w = want[0].copy()
    w["a"] += np.uint32(base)
    w["b"] += np.uint32(base)
    assert len(edges) == len(w) and st["edges"] == len(w), (what, len(edges), len(w), st)
    assert edges.tobytes() == w.tobytes(), (what, edges[:8], w[:8])
    n = st["rows"]
    assert st["rounds"] == want[1] and st["scan_owners"] == want[2] and st["scans"] == len(want[2]), (what, st, want[1:])
    assert st["owner_rows"] == sum(want[2][:want[1]]) and st["pairs"] == sum(want[2]) * n, (what, st)
    if st["rounds"] >= 3:
        assert st["owner_rows"] < st["rounds"] * n, (what, st)


@pytest.mark.parametrize("bits", [128, 160, 512, 1024, 2048, 4096])
def test_parity_with_the_rule(bits):
    """1000 rows: three full owner tiles and a partial one; 160 bits takes the zero-padded copy; the six widths are the six
    instantiations of the fold kernel (4, 8, 16, 32, 64 and 128 words a row)"""
    db, _, S = planted_table(bits)
    t = table(db)
    for cutoff in CUTOFFS:
        want = expected(bits, cutoff)
        assert not_vacuous(bits, cutoff, want), (bits, cutoff, want[1], tied(want[0]), len(want[0]))
        got = t.mst(cutoff)
        same(got, want, (bits, cutoff))
        again = t.mst(cutoff)
        assert again[0].tobytes() == got[0].tobytes(), "two runs give identical bytes"
        assert (again[1]["rounds"], again[1]["scan_owners"]) == (got[1]["rounds"], got[1]["scan_owners"])
        # every cut of the dendrogram at or above the cutoff is gsim_db_components' partition there, byte for byte
        levels = [c for c in LEVELS if c >= cutoff]
        parts, _ = t.components(levels)
        for c, part in zip(levels, parts):
            cut = capi.mst_cut(got[0], N, c)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(cut, part)), (bits, cutoff, c)
        if cutoff >= 0.5:  # the same forest from the neighbour lists and the host function
            assert capi.mst(*t.neighbors(cutoff)).tobytes() == got[0].tobytes(), (bits, cutoff)
    assert tied(expected(bits, TINY)[0]) >= 836
    t.close()


def test_tversky():
    db, _, _ = planted_table(1024)
    S = score_matrix(db, TV)
    t = table(db)
    for cutoff in (0.5, 0.85):
        want = expected(1024, cutoff, TV, S)
        assert want[1] >= 3 and tied(want[0]) >= 600 and len(want[0]) < N - 1
        same(t.mst(cutoff, **TV), want, ("tversky", cutoff))
    assert expected(1024, 0.85, TV, S)[0].tobytes() != expected(1024, 0.85)[0].tobytes(), "Dice is not Tanimoto"
    t.close()


@pytest.mark.parametrize("bits", [160, 1024])
def test_rounds_cut_into_many_launches_give_the_same_bytes(bits):
    db, _, _ = planted_table(bits)
    whole, cut = table(db), table(db, pairs=1)  # one column tile of 256 candidates per launch: 4 launches per scan
    for cutoff in (TINY, 0.5):
        want = expected(bits, cutoff)
        a, sa = whole.mst(cutoff)
        b, sb = cut.mst(cutoff)
        assert sa["launches"] == sa["scans"] and sb["launches"] == 4 * sb["scans"] and sb["scans"] == sa["scans"] >= 3, (sa, sb)
        assert a.tobytes() == b.tobytes(), (bits, cutoff)
        same((b, sb), want, ("cut", bits, cutoff))
    whole.close()
    cut.close()


def test_row_base_and_the_search_state():
    base, cutoff = 7000, 0.5
    db, _, _ = planted_table(2048)
    want = expected(2048, cutoff)
    t = table(db)
    singles = np.ascontiguousarray(db[[3, 500, N - 1]])

    def searches():
        hits, approx = t.search(singles, 50)
        return b"".join(h.tobytes() for h in hits) + approx.tobytes()

    before = searches()
    plain = t.mst(cutoff)
    same(plain, want, "no base")
    assert searches() == before, "the search state is as it was"
    with pytest.raises(capi.GsimError):
        t.mst(1.5)  # a failed call ...
    assert searches() == before
    t.set_row_base(base)
    based = t.mst(cutoff)  # ... and a correct one right after it
    same(based, want, "row base", base=base)
    assert t.mst(cutoff)[0].tobytes() == based[0].tobytes()
    t.close()


def test_edges():
    # 257 rows: one full owner tile and a tile of one row
    db, _, S = planted_table(1024, 257)
    t = table(db)
    for cutoff in (TINY, 0.5, 1.0):
        edges = mst_rule(S, cutoff)
        by_rounds, rounds, scans = boruvka(S, cutoff)
        assert by_rounds.tobytes() == edges.tobytes() and 150 <= len(edges) < 256 and tied(edges) >= 100
        got, st = t.mst(cutoff)
        assert got.tobytes() == edges.tobytes() and (st["rounds"], st["scan_owners"]) == (rounds, scans), (cutoff, st)
    t.close()
    # one row, and no row
    t = table(db[:1])
    got, st = t.mst(0.5)
    assert len(got) == 0 and st["rows"] == 1 and st["launches"] == st["scans"] == st["rounds"] == st["pairs"] == 0
    t.close()
    got, st = capi.Table(1024).mst(0.5)
    assert len(got) == 0 and st["rows"] == 0
    # two rows
    t = table(np.ascontiguousarray(db[[5, 5]]))
    got, st = t.mst(1.0)
    assert got.tolist() == [(0, 1, 1.0)] and st["rounds"] == st["scans"] == 1
    t.close()
    # all rows zero: every score is NaN, nothing is an edge
    t = table(np.zeros((300, 32), np.uint32))
    got, st = t.mst(TINY)
    assert len(got) == 0 and st["rounds"] == 0 and st["scan_owners"] == [300]
    t.close()
    # 600 identical rows: every row's E-first partner is row 0 (row 0's: row 1); one round, and no scan after it: one tree
    t = table(np.repeat(db[7:8], 600, 0))
    got, st = t.mst(1.0)
    assert db[7].any() and len(got) == 599 and np.array_equal(got["a"], np.zeros(599)) and np.array_equal(got["b"], np.arange(1, 600))
    assert (got["score"] == 1.0).all() and st["rounds"] == 1 and st["scan_owners"] == [600]
    t.close()


def test_generated_and_attached_tables():
    """no host copy exists: the expected rows are regenerated with gsim_synth_row; 160 bits attached: a zero-padded copy"""
    import torch
    n, bits, seed = 2000, 1024, 0xC0119
    db = np.stack([capi.synth_row(seed, O.KIND_MORGAN, r, bits) for r in range(n)])
    S = score_matrix(db)
    want = mst_rule(S, 0.3)
    assert 100 <= len(want) < n - 1 and boruvka(S, 0.3)[1] >= 3
    g = capi.Table(bits).generate(seed, O.KIND_MORGAN, 0, n, 0)
    got, st = g.mst(0.3)
    assert got.tobytes() == want.tobytes() and st["rounds"] == boruvka(S, 0.3)[1]
    g.close()
    narrow, _, _ = planted_table(160)
    ten = torch.from_numpy(narrow.view(np.int32).copy()).to("cuda:0")
    a = capi.Table(160)
    a.attach_device_rows(ten.data_ptr(), len(narrow), 0)
    same(a.mst(0.15), expected(160, 0.15), "attached")
    a.close()
