"""DBSCAN density clustering on the GPU (gsim_db_dbscan).

Expected values: the oracle gives the pair scores (tests/test_gpu_components.py's score_matrix) and the rule of include/gpusim_hip.h,
restated in dbscan_rule.py, is applied to them.  Every compared case checks label_of, degree, anchor, first_row, sizes and nclusters and
the stats' kept, cores, borders, noise, clusters and unions, with the identities among them.  Everything is exact: no tolerances.

The tables are 1000 rows -- three full tiles of 256 rows and a partial one, diagonal and off-diagonal -- on a KIND_SPARSE background
with planted structure on rows drawn by one permutation (`planted`):
  (a) 300 identical rows scattered over all tiles (the contended root);
  (b) 3 all-zero rows;
  (c) 8 duplicate pairs;
  (d) up to 5 sliding-window chains of 12 rows in disjoint bit ranges: window w bits, stride w / 8 (w = 16 below 512 bits, else 64), so
      neighbours in a chain score 7/9, rows two apart 0.6, three apart 5/11, four apart 1/3, five apart 3/13;
  (e) at 1024 bits and wider a bridge in the top 160 bits: disjoint bit sets X (32), P (48), Q (48), Y (32); 6 rows = X, 6 rows = Y,
      a* = X u P, b* = Y u Q (b* on a smaller row than a*), R = P u Q, which scores exactly 0.375 against both, and R2 = P u (40 bits
      of Q), which scores 0.4 against a* and 0.3125 against b*.
What the rule makes of it, by hand, at 1024 bits and wider (five chains; `CENSUS`): at (0.3, 5) every chain row has four neighbours or
more and is a core, a* and b* are cores, R and R2 have three neighbours and are the only border rows: R anchors to b* (a tie: the
smaller row), R2 to a* (the better score, on the larger row), in different clusters.  At (0.6, 5) a chain's rows 2 .. 9 are cores and
its rows 0, 1, 10, 11 border rows; at (0.7, 3) its rows 1 .. 10 are cores and its ends border rows.  With the block, the X rows and the
Y rows that is 1 + 5 + 2 = 8 clusters in all three cases.  (The feature request's table had 353 / 19 / 628 / 7 at (0.6, 5) and 7
clusters at (0.3, 5); counted by hand and by dbscan_rule this recipe gives 352 / 20 / 628 / 8 and 8.  Its other figures, and those
for 128 and 160 bits -- 12 and 16 border rows, 4 and 5 clusters at (0.6, 5) -- are the ones found here.)

Non-vacuity, asserted on the EXPECTED result of every compared case on these tables (`not_vacuous`): at least 4 clusters, at least 100
noise rows, one cluster of at least 100 rows with members in at least 3 tiles; at least 6 border rows wherever the rule allows any
beside the bridge's: with min_pts == 2 a row with a neighbour is a core, so there are none, and at (0.3, 5) all chain rows are cores and
the bridge's two are all there is (none below 1024 bits); there the bridge is asserted instead: a border row whose best-scoring core
neighbours lie in two clusters, and one whose core neighbours in two clusters differ in score."""
import numpy as np
import pytest

import oracle_lib as O
from gpusimilarity_amd import capi
from components_rule import components_rule
from dbscan_rule import NOISE, census, dbscan_rule
from test_gpu_components import TILE, TV, knobs, score_matrix, window_row

pytestmark = pytest.mark.gpu
PAIRS = "GSIM_DBSCAN_LAUNCH_PAIRS"
CASES = ((0.3, 5), (0.6, 5), (0.7, 3), (0.5, 2), (1.0, 2))
# (cores, borders, noise, clusters) at 1024 bits and wider, by hand (the module's docstring)
CENSUS = {(0.3, 5): (374, 2, 624, 8), (0.6, 5): (352, 20, 628, 8), (0.7, 3): (362, 10, 628, 8)}
COMPARED = [0]


def table(db, pairs=None, base=0):
    with knobs(**{PAIRS: pairs}):
        t = capi.Table(db.shape[1] * 32).add_rows(db).finalize(0, 1)
    if base:
        t.set_row_base(base)
    return t


def bits_row(W, bits):
    row = np.zeros(W, np.uint32)
    for bit in bits:
        row[bit // 32] |= np.uint32(1 << (bit % 32))
    return row


def planted(db, rng):
    """Plants (a) .. (e) of the module's docstring on rows drawn by one permutation.  Returns a dict of the planted rows."""
    n, W = db.shape
    nbits = W * 32
    where = iter(rng.permutation(n).tolist())
    take = lambda k: [next(where) for _ in range(k)]
    rows = {}
    rows["block"] = take(300)
    db[rows["block"]] = db[rows["block"][0]] if db[rows["block"][0]].any() else window_row(W, 3, 40)
    rows["zero"] = take(3)
    db[rows["zero"]] = 0
    rows["dup"] = take(16)
    for k in range(8):
        db[rows["dup"][2 * k + 1]] = db[rows["dup"][2 * k]]
    w = 16 if nbits < 512 else 64
    span = w + 11 * (w // 8)  # bits a chain of 12 covers
    room = nbits - 160 if nbits >= 1024 else nbits
    rows["chains"] = []
    for c in range(min(5, room // span)):
        links = take(12)
        for t, r in enumerate(links):
            db[r] = window_row(W, c * span + t * (w // 8), w)
        rows["chains"].append(links)
    if nbits >= 1024:
        top = nbits - 160
        X, P, Q, Y = range(top, top + 32), range(top + 32, top + 80), range(top + 80, top + 128), range(top + 128, top + 160)
        rows["X"], rows["Y"] = take(6), take(6)
        db[rows["X"]] = bits_row(W, X)
        db[rows["Y"]] = bits_row(W, Y)
        four = sorted(take(4))
        rows["b*"], rows["a*"], rows["R"], rows["R2"] = four[0], four[2], four[1], four[3]  # b* on a smaller row than a*
        db[rows["a*"]] = bits_row(W, list(X) + list(P))
        db[rows["b*"]] = bits_row(W, list(Y) + list(Q))
        db[rows["R"]] = bits_row(W, list(P) + list(Q))
        db[rows["R2"]] = bits_row(W, list(P) + list(Q)[:40])
    return rows


_TABLES = {}


def planted_table(bits, n=1000):
    """(rows, the planted rows, the oracle's Tanimoto scores) of the planted table of that width: made once, never changed"""
    if (bits, n) not in _TABLES:
        W = bits // 32
        rng = np.random.default_rng(bits * 11 + n)
        db = O.synth_rows(0xDB5CA + bits, O.KIND_SPARSE, 0, n, W)
        rows = planted(db, rng)
        S = score_matrix(db)
        for x in (db, S):
            x.setflags(write=False)
        _TABLES[(bits, n)] = (db, rows, S)
    return _TABLES[(bits, n)]


_WANT = {}


def expected(bits, cutoff, min_pts):
    if (bits, cutoff, min_pts) not in _WANT:
        _WANT[(bits, cutoff, min_pts)] = dbscan_rule(planted_table(bits)[2], cutoff, min_pts)
    return _WANT[(bits, cutoff, min_pts)]


def core_neighbours(S, want, cutoff, x):
    """the core neighbours of row x with their scores, as the rule sees them (a pair's score comes from its smaller row)"""
    _, _, anchor, _, _, _ = want
    n = len(anchor)
    out = []
    for c in range(n):
        s = S[min(x, c), max(x, c)]
        if c != x and anchor[c] == c and s >= np.float32(cutoff):
            out.append((c, float(s)))
    return out


def bridge_is_there(S, want, cutoff, rows):
    label_of, _, anchor, _, _, _ = want
    R, R2, a, b = rows["R"], rows["R2"], rows["a*"], rows["b*"]
    assert b < a and S[min(R, a), max(R, a)] == np.float32(0.375) == S[min(R, b), max(R, b)]
    assert S[min(R2, a), max(R2, a)] == np.float32(0.4) and S[min(R2, b), max(R2, b)] == np.float32(0.3125)
    near = core_neighbours(S, want, cutoff, R)
    top = [c for c, s in near if s == max(s for _, s in near)]
    tie = sorted(top) == [b, a] and label_of[a] != label_of[b] and anchor[R] == b and label_of[R] == label_of[b]
    near2 = dict(core_neighbours(S, want, cutoff, R2))
    better = set(near2) == {a, b} and near2[a] > near2[b] and anchor[R2] == a and label_of[R2] == label_of[a] != label_of[R]
    return tie and better


def not_vacuous(bits, cutoff, min_pts):
    db, rows, S = planted_table(bits)
    want = expected(bits, cutoff, min_pts)
    label_of, _, _, first_row, sizes, _ = want
    cores, borders, noise, clusters = census(want)
    big = [c for c in np.flatnonzero(sizes >= 100) if len(np.unique(np.flatnonzero(label_of == c) // TILE)) >= 3]
    ok = clusters >= 4 and noise >= 100 and len(big) >= 1
    if min_pts == 2:
        ok = ok and borders == 0  # (a row with a neighbour is a core)
    elif (cutoff, min_pts) == (0.3, 5):
        ok = ok and (bits < 1024 or (borders >= 2 and bridge_is_there(S, want, cutoff, rows)))
    else:
        ok = ok and borders >= 6
    if bits >= 1024 and (cutoff, min_pts) in CENSUS:
        ok = ok and census(want) == CENSUS[(cutoff, min_pts)]
    if bits in (128, 160) and (cutoff, min_pts) == (0.6, 5):  # three and four chains, no bridge
        ok = ok and (borders, clusters) == {128: (12, 4), 160: (16, 5)}[bits]
    return ok


def same(got, want, what, base=0):
    label_of, degree, anchor, first_row, sizes, st = got
    n = len(label_of)
    real = want[2] != NOISE
    assert np.array_equal(label_of, want[0]), (what, np.flatnonzero(label_of != want[0])[:10])
    assert np.array_equal(degree, want[1]), (what, np.flatnonzero(degree != want[1])[:10])
    assert np.array_equal(anchor, np.where(real, want[2] + np.uint32(base), NOISE).astype(np.uint32)), (what, np.flatnonzero(anchor != want[2])[:10])
    assert np.array_equal(first_row, want[3] + np.uint32(base)), (what, first_row[:20], want[3][:20])
    assert np.array_equal(sizes, want[4]), (what, sizes[:20], want[4][:20])
    cores, borders, noise, clusters = census(want)
    assert st["rows"] == n and st["pairs"] == n * (n - 1) // 2, (what, st)
    assert (st["kept"], st["cores"], st["borders"], st["noise"], st["clusters"]) == (want[5], cores, borders, noise, clusters), (what, st)
    # the identities the host verifies
    assert int(degree.sum(dtype=np.uint64)) == 2 * st["kept"] and st["unions"] == st["cores"] - st["clusters"], (what, st)
    assert st["cores"] + st["borders"] + st["noise"] == n and int(sizes.sum()) == cores + borders, (what, st)
    COMPARED[0] += 1


def as_bytes(got):
    return b"".join(x.tobytes() for x in got[:5])


@pytest.mark.parametrize("bits", [128, 160, 512, 1024, 2048, 4096])
def test_parity_with_the_rule(bits):
    """the six widths are the six instantiations of both tile kernels (4, 8, 16, 32, 64 and 128 words a row); 160 bits takes the
    zero-padded copy"""
    db, rows, S = planted_table(bits)
    t = table(db)
    for cutoff, min_pts in CASES:
        want = expected(bits, cutoff, min_pts)
        print(bits, cutoff, min_pts, "cores, borders, noise, clusters:", census(want))
        assert not_vacuous(bits, cutoff, min_pts), (bits, cutoff, min_pts, census(want), np.sort(want[4])[-6:])
        got = t.dbscan(cutoff, min_pts)
        assert got[5]["launches_count"] == got[5]["launches_link"] == 1
        same(got, want, (bits, cutoff, min_pts))
        again = t.dbscan(cutoff, min_pts)
        assert as_bytes(again) == as_bytes(got), "two runs give identical bytes"
        assert all(again[5][k] == got[5][k] for k in ("kept", "cores", "borders", "noise", "clusters", "unions"))
        # the same answer from the neighbour lists and the host function
        host = capi.dbscan(*t.neighbors(cutoff), min_pts)
        assert b"".join(x.tobytes() for x in host) == b"".join(got[k].tobytes() for k in (0, 2, 3, 4)), (bits, cutoff, min_pts)
        # restricted to the cores, the partition is gsim_components' on the core-induced subgraph
        cores = np.flatnonzero(want[2] == np.arange(len(db)))
        sub = components_rule(S[np.ix_(cores, cores)], cutoff)
        assert np.array_equal(got[0][cores], sub[0]) and np.array_equal(got[3], cores[sub[1]])
    print("dbscan calls compared with the rule so far:", COMPARED[0])
    t.close()


def test_min_pts_one_equals_the_components():
    db, _, S = planted_table(1024)
    t = table(db)
    for cutoff in (0.3, 0.7, 1.0):
        label_of, degree, anchor, first_row, sizes, st = t.dbscan(cutoff, 1)
        (component_of, cfirst, csizes), = t.components(cutoff)[0]
        assert label_of.tobytes() == component_of.tobytes() and first_row.tobytes() == cfirst.tobytes() and sizes.tobytes() == csizes.tobytes()
        assert np.array_equal(anchor, np.arange(1000)) and st["cores"] == 1000 and st["borders"] == st["noise"] == 0
        same((label_of, degree, anchor, first_row, sizes, st), dbscan_rule(S, cutoff, 1), ("min_pts 1", cutoff))
        assert label_of[planted_table(1024)[1]["zero"]].tolist() != [NOISE] * 3, "all-zero rows are cores of their own"
    t.close()


def test_more_points_than_rows_is_all_noise():
    db, _, _ = planted_table(1024)
    t = table(db)
    label_of, degree, anchor, first_row, sizes, st = t.dbscan(0.6, 1001)
    assert (label_of == NOISE).all() and (anchor == NOISE).all() and len(first_row) == len(sizes) == 0
    assert np.array_equal(degree, expected(1024, 0.6, 5)[1]) and st["cores"] == st["clusters"] == st["unions"] == 0 and st["noise"] == 1000
    t.close()


def test_tversky():
    db, _, _ = planted_table(1024)
    S = score_matrix(db, TV)
    t = table(db)
    for cutoff, min_pts in ((0.75, 5), (0.82, 3)):  # Dice of 0.6 and 0.7
        want = dbscan_rule(S, cutoff, min_pts)
        cores, borders, noise, clusters = census(want)
        assert clusters >= 4 and borders >= 6 and noise >= 100, census(want)
        same(t.dbscan(cutoff, min_pts, **TV), want, ("tversky", cutoff, min_pts))
    assert census(dbscan_rule(S, 0.7, 3)) != census(expected(1024, 0.7, 3)), "Dice is not Tanimoto"
    t.close()


def test_row_base_the_search_state_and_the_outputs_not_asked_for():
    n, base, cutoff, min_pts = 1000, 7000, 0.6, 5
    db, _, _ = planted_table(2048)
    want = expected(2048, cutoff, min_pts)
    assert not_vacuous(2048, cutoff, min_pts)
    t = table(db)
    singles = np.ascontiguousarray(db[[3, 500, n - 1]])

    def searches():
        hits, approx = t.search(singles, 50)
        return b"".join(h.tobytes() for h in hits) + approx.tobytes()

    before = searches()
    plain = t.dbscan(cutoff, min_pts)
    same(plain, want, "no base")
    assert searches() == before, "the search state is as it was"
    with pytest.raises(capi.GsimError):
        t.dbscan(cutoff, 0)  # a failed call ...
    with pytest.raises(capi.GsimError):
        t.dbscan(1.5, min_pts)
    assert searches() == before
    t.set_row_base(base)
    based = t.dbscan(cutoff, min_pts)  # ... and a correct one right after it
    same(based, want, "row base", base=base)
    assert np.array_equal(based[0], plain[0]), "label_of does not carry the row base"
    assert np.array_equal(based[3], plain[3] + np.uint32(base)), "first_row does"
    real = plain[2] != NOISE
    assert np.array_equal(based[2][real], plain[2][real] + np.uint32(base)) and (based[2][~real] == NOISE).all(), "anchor does, noise stays noise"
    bare = t.dbscan(cutoff, min_pts, degree=False, anchor=False, first_row=False, sizes=False)
    assert bare[1:5] == (None, None, None, None) and np.array_equal(bare[0], plain[0])
    assert all(bare[5][k] == plain[5][k] for k in ("kept", "cores", "borders", "noise", "clusters", "unions"))
    some = t.dbscan(cutoff, min_pts, degree=False, first_row=False)
    assert some[1] is None and some[3] is None and np.array_equal(some[2], based[2]) and np.array_equal(some[4], plain[4])
    t.close()


@pytest.mark.parametrize("bits", [160, 1024])
def test_passes_cut_into_many_launches_give_the_same_bytes(bits):
    db, _, _ = planted_table(bits)
    whole, cut, three = table(db), table(db, pairs=TILE * TILE), table(db, pairs=3 * TILE * TILE)
    for cutoff, min_pts in ((0.6, 5), (0.3, 5), (0.7, 3)):
        assert not_vacuous(bits, cutoff, min_pts)
        a, b, c = whole.dbscan(cutoff, min_pts), cut.dbscan(cutoff, min_pts), three.dbscan(cutoff, min_pts)
        # one tile per launch: the ten tiles of the triangle; three per launch: tile rows of 4, 3, 2 and 1 tiles give 3 + 1, 3, and
        # 2 + 1 together
        assert [(x[5]["launches_count"], x[5]["launches_link"]) for x in (a, b, c)] == [(1, 1), (10, 10), (4, 4)]
        assert as_bytes(a) == as_bytes(b) == as_bytes(c), (bits, cutoff, min_pts)
        same(b, expected(bits, cutoff, min_pts), ("one tile per launch", bits, cutoff, min_pts))
        same(c, expected(bits, cutoff, min_pts), ("three tiles per launch", bits, cutoff, min_pts))
    for t in (whole, cut, three):
        t.close()


def test_edges():
    # 257 rows: one full tile and a tile of one row
    db = np.array(planted_table(1024)[0][:257])
    db[256] = planted_table(1024)[0][planted_table(1024)[1]["block"][0]]  # the lone row of the second tile belongs to the block
    S = score_matrix(db)
    t = table(db)
    for cutoff, min_pts in ((0.6, 5), (1.0, 3)):
        want = dbscan_rule(S, cutoff, min_pts)
        cores, borders, noise, clusters = census(want)
        assert cores >= 50 and noise >= 50 and clusters >= 1 and want[0][256] != NOISE, census(want)
        same(t.dbscan(cutoff, min_pts), want, (257, cutoff, min_pts))
    t.close()
    # one row
    t = table(db[:1])
    label_of, degree, anchor, first_row, sizes, st = t.dbscan(0.5, 1)
    assert label_of.tolist() == [0] and degree.tolist() == [0] and anchor.tolist() == [0] and first_row.tolist() == [0] and sizes.tolist() == [1]
    assert st["launches_count"] == st["launches_link"] == 0 and st["pairs"] == st["kept"] == st["unions"] == 0 and st["cores"] == 1
    label_of, degree, anchor, first_row, sizes, st = t.dbscan(0.5, 2)
    assert label_of.tolist() == [NOISE] and anchor.tolist() == [NOISE] and len(first_row) == 0 and st["noise"] == 1
    t.close()
    # all rows zero: all noise for min_pts >= 2, 300 singleton clusters at 1
    t = table(np.zeros((300, 32), np.uint32))
    label_of, degree, anchor, first_row, sizes, st = t.dbscan(0.01, 2)
    assert (label_of == NOISE).all() and not degree.any() and len(first_row) == 0 and st["noise"] == 300 and st["kept"] == 0
    label_of, degree, anchor, first_row, sizes, st = t.dbscan(0.01, 1)
    assert np.array_equal(label_of, np.arange(300)) and np.array_equal(first_row, np.arange(300)) and (sizes == 1).all()
    assert st["cores"] == st["clusters"] == 300 and st["unions"] == 0 and st["pairs"] == 300 * 299 // 2
    t.close()
    # all rows identical: one cluster, through the contended root
    t = table(np.repeat(db[256:], 700, 0))
    for min_pts in (1, 5, 700):
        label_of, degree, anchor, first_row, sizes, st = t.dbscan(1.0, min_pts)
        assert not label_of.any() and (degree == 699).all() and first_row.tolist() == [0] and sizes.tolist() == [700]
        assert st["kept"] == 700 * 699 // 2 and st["unions"] == 699 and st["cores"] == 700
    assert (t.dbscan(1.0, 701)[0] == NOISE).all()
    t.close()
    COMPARED[0] += 1


def test_a_generated_table():
    """no host copy exists: the expected rows are regenerated with gsim_synth_row"""
    n, bits, seed = 2000, 1024, 0xC0119
    db = np.stack([capi.synth_row(seed, O.KIND_MORGAN, r, bits) for r in range(n)])
    S = score_matrix(db)
    generated = capi.Table(bits).generate(seed, O.KIND_MORGAN, 0, n, 0)
    seen = set()
    for cutoff, min_pts in ((0.3, 4), (0.25, 10), (0.3, 20)):
        want = dbscan_rule(S, cutoff, min_pts)
        cores, borders, noise, clusters = census(want)
        print("generated", cutoff, min_pts, census(want))
        assert cores >= 10 and borders >= 6 and noise >= 100 and clusters >= 1, census(want)
        seen.add(census(want))
        same(generated.dbscan(cutoff, min_pts), want, ("generated", cutoff, min_pts))
    assert len(seen) == 3
    generated.close()


def test_enough_cases_were_compared():
    assert COMPARED[0] >= 6 * 5 + 3 + 2 + 2 + 2 * 6 + 2 + 1 + 3, COMPARED[0]
