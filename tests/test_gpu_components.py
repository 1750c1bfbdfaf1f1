"""Single-linkage clustering on the GPU (gsim_db_components).

Expected values: the oracle gives the pair scores -- oracle_lib.tanimoto_raw, or oracle_lib.search(row, table, k = n, cutoff = 0) for
Tversky -- and the rule of include/gpusim_hip.h, restated in components_rule.py, is applied to them.  Every compared case checks
`component_of`, `ncomponents`, `first_row`, `sizes`, `stats.kept` and `stats.unions`.  Everything is exact: no tolerances.

Non-vacuity (`not_vacuous`), asserted on the EXPECTED result of every compared case on the planted 1000-row tables: at least 5
components with more than one member, at least one component of at least 100 rows with members in at least 3 tiles of 256 rows, and
fewer components than rows (the tests of single edges -- 257 rows, one row, all rows zero, the generated table -- say what they expect
instead; so does cutoff 0.15 on the 128- and 160-bit tables, where sparse rows DO pair up by themselves and all but a few rows merge
into one giant component: `merged`).  Tables carry planted structure (`planted`), because sparse rows wider than 128 bits have no pair above 0.15 by themselves:
duplicates, zero rows and near-copies, a sliding-window chain scattered over all tiles (one component at 0.7 whose end rows score 0.0
against each other) and a block of 600 identical rows spread over all tiles (the contended root)."""
import contextlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as O
from gpusimilarity_amd import capi
from components_rule import components_rule, refines

pytestmark = pytest.mark.gpu
NT = 16
PAIRS = "GSIM_COMPONENTS_LAUNCH_PAIRS"
TILE = 256
TAN = dict()
TV = dict(metric=capi.METRIC_TVERSKY, alpha=0.5, beta=0.5)
CUTOFFS = (0.15, 0.5, 0.7, 1.0)
LEVELS = (0.15, 0.3, 0.5, 0.6, 0.7, 0.8, 0.95, 1.0)
COMPARED = [0]


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


def table(db, pairs=None, base=0):
    with knobs(**{PAIRS: pairs}):
        t = capi.Table(db.shape[1] * 32).add_rows(db).finalize(0, 1)
    if base:
        t.set_row_base(base)
    return t


def window_row(W, first_bit, nbits=64):
    row = np.zeros(W, np.uint32)
    for bit in range(first_bit, first_bit + nbits):
        row[bit // 32] |= np.uint32(1 << (bit % 32))
    return row


def planted(db, rng, block=600, chain=100):
    """tests/test_gpu_leader.py's duplicates, three all-zero rows and twenty near-copies with a few bits flipped; then, on rows of
    their own drawn by one permutation of the table, `block` identical rows and a chain: its row t has the bits [8 t, 8 t + 64) set, so
    neighbours in the chain score 56 / 72, rows two apart 48 / 80, and rows eight or more apart 0.  Returns the chain's rows in
    chain order.  Eight more duplicate pairs go on rows that nothing else overwrites."""
    n, W = db.shape
    for i in rng.choice(n, 6, replace=False):
        db[int(rng.integers(n))] = db[i]
    db[rng.choice(n, 3, replace=False)] = 0
    for i in rng.choice(n, 20, replace=False):
        j = int(rng.integers(n))
        db[j] = db[i]
        for bit in rng.choice(W * 32, 3, replace=False):
            db[j, bit // 32] ^= np.uint32(1 << (bit % 32))
    chain = min(chain, (W * 32 - 64) // 8 + 1)
    where = rng.permutation(n)
    db[where[:block]] = db[where[0]] if db[where[0]].any() else window_row(W, 3, 40)
    links = where[block:block + chain]
    for t, r in enumerate(links):
        db[r] = window_row(W, 8 * t)
    rest = where[block + chain:]
    for k in range(8):  # eight more duplicate pairs, on rows nothing above overwrites
        db[rest[2 * k + 1]] = db[rest[2 * k]]
    return links


def score_matrix(db, kw=TAN):
    """S[p, i] = score(query = row p, row i) from the oracle: NaN (Tanimoto, raw) or 0 (Tversky, through the search) for 0 / 0 --
    neither is ever >= a cutoff in (0, 1]."""
    n = len(db)
    S = np.empty((n, n), np.float32)
    if kw.get("metric", capi.METRIC_TANIMOTO) == capi.METRIC_TANIMOTO:
        with ThreadPoolExecutor(NT) as pool:
            list(pool.map(lambda r: S.__setitem__(r, O.tanimoto_raw(db[r], db)[0]), range(n)))
    else:
        def tversky(r):
            hits, _ = O.search(db[r], db, n, 0.0, O.METRIC_TVERSKY, kw["alpha"], kw["beta"])
            S[r] = 0
            S[r, hits["row"]] = hits["score"]
        with ThreadPoolExecutor(NT) as pool:
            list(pool.map(tversky, range(n)))
    return S


_TABLES = {}


def planted_table(bits, n=1000):
    """(rows, the chain's rows, the oracle's Tanimoto scores) of the planted sparse table of that width: made once, never changed"""
    if (bits, n) not in _TABLES:
        W = bits // 32
        rng = np.random.default_rng(bits * 7 + n)
        db = O.synth_rows(0xC0117 + bits, O.KIND_SPARSE, 0, n, W)
        links = planted(db, rng, block=n * 3 // 5, chain=n // 10)
        S = score_matrix(db)
        for x in (db, links, S):
            x.setflags(write=False)
        _TABLES[(bits, n)] = (db, links, S)
    return _TABLES[(bits, n)]


def not_vacuous(want, n):
    component_of, first_row, sizes, _ = want
    big = [c for c in np.flatnonzero(sizes >= 100) if len(np.unique(np.flatnonzero(component_of == c) // TILE)) >= 3]
    return int((sizes > 1).sum()) >= 5 and len(big) >= 1 and len(first_row) < n


def merged(want, n):
    """rows of at most 160 bits at 0.15: one giant component over all four tiles, a few rows left out of it"""
    component_of, first_row, sizes, _ = want
    giant = int(np.argmax(sizes))
    return sizes[giant] >= 900 and len(np.unique(np.flatnonzero(component_of == giant) // TILE)) == 4 and 1 < len(first_row) < n


def same(level, st, want, what, base=0):
    component_of, first_row, sizes = level
    assert np.array_equal(component_of, want[0]), (what, component_of[:20], want[0][:20])
    assert np.array_equal(first_row, want[1] + np.uint32(base)), (what, first_row[:20], want[1][:20])
    assert np.array_equal(sizes, want[2]), (what, sizes[:20], want[2][:20])
    n = len(component_of)
    assert st["rows"] == n and st["pairs"] == n * (n - 1) // 2, (what, st)
    if st["levels"] == 1:
        assert st["kept"] == want[3] and st["unions"] == n - len(want[1]), (what, st, want[3], len(want[1]))
    COMPARED[0] += 1


def as_bytes(level):
    return b"".join(x.tobytes() for x in level)


@pytest.mark.parametrize("bits", [128, 160, 512, 1024, 2048, 4096])
def test_parity_with_the_oracle(bits):
    """1000 rows: three full tiles and a partial one, diagonal and off-diagonal; 160 bits takes the zero-padded copy; the six widths
    are the six instantiations of the tile kernel (4, 8, 16, 32, 64 and 128 words a row)"""
    n = 1000
    db, links, S = planted_table(bits)
    t = table(db)
    for cutoff in CUTOFFS:
        want = components_rule(S, cutoff)
        ok = merged(want, n) if bits <= 160 and cutoff == 0.15 else not_vacuous(want, n)
        assert ok, (bits, cutoff, len(want[1]), np.sort(want[2])[-6:])
        levels, st = t.components(cutoff)
        assert len(levels) == 1 and st["levels"] == 1 and st["launches"] == 1
        same(levels[0], st, want, (bits, cutoff))
        again, st2 = t.components([cutoff])
        assert as_bytes(again[0]) == as_bytes(levels[0]), "two runs give identical bytes"
        assert (st2["kept"], st2["unions"]) == (st["kept"], st["unions"])
        # the same partition from the neighbour lists and the host function
        got = capi.components(*t.neighbors(cutoff)[:2])
        assert as_bytes(got) == as_bytes(levels[0]), (bits, cutoff)
    if bits >= 1024:  # the chain: one component at 0.7 although its ends have no bit in common
        want = components_rule(S, 0.7)
        assert S[links[0], links[-1]] == 0.0 and len(links) == 100
        assert len(set(want[0][links].tolist())) == 1 and want[2][want[0][links[0]]] == len(links)
        assert len(np.unique(links // TILE)) == 4, "scattered over all tiles"
    print("components calls compared with the oracle so far:", COMPARED[0])
    t.close()


def test_eight_levels_in_one_pass_equal_eight_calls():
    n = 1000
    db, _, S = planted_table(1024)
    t = table(db)
    levels, st = t.components(LEVELS)
    assert len(levels) == 8 and st["levels"] == 8 and st["launches"] == 1
    wants = [components_rule(S, c) for c in LEVELS]
    assert all(not_vacuous(w, n) for w in wants)
    assert len(set(len(w[1]) for w in wants)) >= 3, "the number of components differs between at least 3 of the levels"
    assert st["kept"] == wants[0][3] and st["unions"] == sum(n - len(w[1]) for w in wants), st
    for l, cutoff in enumerate(LEVELS):
        same(levels[l], st, wants[l], ("level", l))
        single, _ = t.components(cutoff)
        assert as_bytes(single[0]) == as_bytes(levels[l]), ("a single-level call and the stripe of the multi-level call", l)
        if l:
            assert refines(levels[l][0], levels[l - 1][0]), l
    # the outputs that were not asked for
    bare, st2 = t.components(LEVELS, first_row=False, sizes=False)
    assert all(b[1] is None and b[2] is None and np.array_equal(b[0], lv[0]) for b, lv in zip(bare, levels))
    assert st2["unions"] == st["unions"]
    t.close()


def test_tversky():
    n = 1000
    db, _, _ = planted_table(1024)
    S = score_matrix(db, TV)
    t = table(db)
    for cutoff in (0.5, 0.85):
        want = components_rule(S, cutoff)
        assert not_vacuous(want, n)
        levels, st = t.components(cutoff, **TV)
        same(levels[0], st, want, ("tversky", cutoff))
    assert len(components_rule(S, 0.85)[1]) != len(components_rule(planted_table(1024)[2], 0.85)[1]), "Dice is not Tanimoto"
    t.close()


def test_row_base_and_the_search_state():
    n, base, cutoff = 1000, 7000, 0.7
    db, _, S = planted_table(2048)
    want = components_rule(S, cutoff)
    t = table(db)
    singles = np.ascontiguousarray(db[[3, 500, n - 1]])

    def searches():
        hits, approx = t.search(singles, 50)
        return b"".join(h.tobytes() for h in hits) + approx.tobytes()

    before = searches()
    plain, st = t.components(cutoff)
    same(plain[0], st, want, "no base")
    assert searches() == before, "the search state is as it was"
    with pytest.raises(capi.GsimError):
        t.components([0.7, 0.5])  # a failed call ...
    assert searches() == before
    t.set_row_base(base)
    based, st = t.components(cutoff)  # ... and a correct one right after it
    same(based[0], st, want, "row base", base=base)
    assert np.array_equal(based[0][0], plain[0][0]), "component_of does not carry the row base"
    assert np.array_equal(based[0][1], plain[0][1] + np.uint32(base)), "first_row does"
    t.close()


@pytest.mark.parametrize("bits", [160, 1024])
def test_a_pass_cut_into_many_launches_gives_the_same_bytes(bits):
    n = 1000
    db, _, S = planted_table(bits)
    whole, cut = table(db), table(db, pairs=TILE * TILE)  # one tile per launch: the ten tiles of the triangle
    for cutoffs in ([0.15], [0.7], list(LEVELS)):
        assert bits <= 160 or not_vacuous(components_rule(S, cutoffs[0]), n)
        a, sa = whole.components(cutoffs)
        b, sb = cut.components(cutoffs)
        assert sa["launches"] == 1 and sb["launches"] == 10, (sa, sb)
        assert [as_bytes(x) for x in a] == [as_bytes(x) for x in b], (bits, cutoffs)
        assert (sa["kept"], sa["unions"]) == (sb["kept"], sb["unions"])
        if len(cutoffs) == 1:
            same(b[0], sb, components_rule(S, cutoffs[0]), ("cut", bits, cutoffs))
    three = table(db, pairs=3 * TILE * TILE)
    c, sc = three.components([0.5])
    assert sc["launches"] == 4  # tile rows of 4, 3, 2 and 1 tiles at three tiles per launch: 3 + 1, 3, and 2 + 1 together
    same(c[0], sc, components_rule(S, 0.5), ("three tiles per launch", bits))
    for t in (whole, cut, three):
        t.close()


def test_edges():
    # 257 rows: one full tile and a tile of one row
    db, links, S = planted_table(1024, 257)
    t = table(db)
    for cutoff in (0.5, 1.0):
        want = components_rule(S, cutoff)
        assert int((want[2] > 1).sum()) >= 3 and want[2].max() >= 150 and len(want[1]) < 257
        levels, st = t.components(cutoff)
        same(levels[0], st, want, (257, cutoff))
    assert len(set(components_rule(S, 0.7)[0][links].tolist())) == 1 and len(links) == 25
    t.close()
    # one row
    t = table(db[:1])
    levels, st = t.components([0.3, 0.9])
    for component_of, first_row, sizes in levels:
        assert component_of.tolist() == [0] and first_row.tolist() == [0] and sizes.tolist() == [1]
    assert st["launches"] == 0 and st["pairs"] == st["kept"] == st["unions"] == 0
    t.close()
    # all rows zero: every row a singleton at every level
    t = table(np.zeros((300, 32), np.uint32))
    levels, st = t.components([0.01, 1.0])
    for component_of, first_row, sizes in levels:
        assert np.array_equal(component_of, np.arange(300)) and np.array_equal(first_row, np.arange(300)) and (sizes == 1).all()
    assert st["kept"] == st["unions"] == 0 and st["pairs"] == 300 * 299 // 2
    t.close()
    # all rows identical: one component, through the contended root
    t = table(np.repeat(db[links[:1]], 700, 0))
    levels, st = t.components(1.0)
    assert not levels[0][0].any() and levels[0][1].tolist() == [0] and levels[0][2].tolist() == [700]
    assert st["kept"] == 700 * 699 // 2 and st["unions"] == 699
    t.close()


def test_a_generated_table():
    """no host copy exists: the expected rows are regenerated with gsim_synth_row"""
    n, bits, seed = 2000, 1024, 0xC0119
    db = np.stack([capi.synth_row(seed, O.KIND_MORGAN, r, bits) for r in range(n)])
    S = score_matrix(db)
    generated = capi.Table(bits).generate(seed, O.KIND_MORGAN, 0, n, 0)
    cutoffs = (0.3, 0.45, 0.6)
    wants = [components_rule(S, c) for c in cutoffs]
    assert all(int((w[2] > 1).sum()) >= 5 and len(w[1]) < n for w in wants), [np.sort(w[2])[-5:] for w in wants]
    assert len(set(len(w[1]) for w in wants)) == 3
    levels, st = generated.components(cutoffs)
    assert st["launches"] == 1 and st["unions"] == sum(n - len(w[1]) for w in wants) and st["kept"] == wants[0][3]
    for l in range(3):
        same(levels[l], st, wants[l], ("generated", l))
    generated.close()


def test_enough_cases_were_compared():
    assert COMPARED[0] >= 12, COMPARED[0]
