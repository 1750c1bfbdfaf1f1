"""Leader (sphere-exclusion) clustering on the GPU (gsim_db_leader).

Expected values: the oracle gives the pair scores -- oracle_lib.tanimoto_raw, or oracle_lib.search(row, table, k = n, cutoff = 0) for
Tversky -- and the rule of include/gpusim_hip.h, restated in leader_rule.py, is applied to them.  Every compared case checks
`leaders`, their number, `leader_of` and the bits of `row_score`.  Everything is exact: no tolerances.

Non-vacuity: a compared case must have, in the EXPECTED result, at least 5 clusters with more than one member, at least 5 leaders, and
fewer leaders than rows (the tests of single edges -- one row, all rows identical, all rows zero -- say what they expect instead).
Tables carry planted structure (`planted`), because sparse rows wider than 128 bits have no pair above 0.15 by themselves."""
import contextlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as O
from gpusimilarity_amd import capi
from leader_rule import NONE, leader_rule

pytestmark = pytest.mark.gpu
NT = 16
ROUND, PAIRS = "GSIM_LEADER_ROUND", "GSIM_LEADER_LAUNCH_PAIRS"
DEFAULT_ROUND = 256
TAN = dict()
TV = dict(metric=capi.METRIC_TVERSKY, alpha=0.5, beta=0.5)
CUTOFFS = (0.15, 0.34, 0.5, 0.7)
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


def table(db, round=None, pairs=None, base=0):
    with knobs(**{ROUND: round, PAIRS: pairs}):
        t = capi.Table(db.shape[1] * 32).add_rows(db).finalize(0, 1)
    if base:
        t.set_row_base(base)
    return t


def planted(db, rng):
    """duplicates, three all-zero rows, a block of 40 identical rows, twenty near-copies with a few bits flipped"""
    n, W = db.shape
    for i in rng.choice(n, 6, replace=False):
        db[int(rng.integers(n))] = db[i]
    db[rng.choice(n, 3, replace=False)] = 0
    b = int(rng.integers(0, n - 40))
    db[b:b + 40] = db[b]
    for i in rng.choice(n, 20, replace=False):
        j = int(rng.integers(n))
        db[j] = db[i]
        for bit in rng.choice(W * 32, 3, replace=False):
            db[j, bit // 32] ^= np.uint32(1 << (bit % 32))
    return db, b


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


def rule(S, cutoff, seeds=(), max_leaders=None):
    return leader_rule(lambda r: S[r], S.shape[0], cutoff, seeds, max_leaders)


def not_vacuous(want):
    leaders, leader_of = want[0], want[1]
    sizes = np.bincount(leader_of[leader_of != NONE], minlength=len(leaders))
    return int((sizes > 1).sum()) >= 5 and 5 <= len(leaders) < len(leader_of)


def same(got, want, what, base=0):
    leaders, leader_of, row_score, st = got
    assert np.array_equal(leaders, want[0] + np.uint32(base)), (what, leaders[:20], want[0][:20])
    assert st["leaders"] == len(want[0]), what
    if leader_of is not None:
        assert np.array_equal(leader_of, want[1]), what
        assert np.array_equal(row_score.view(np.uint32), want[2].view(np.uint32)), what
    assert st["assigned"] == int(np.count_nonzero(want[1] != NONE)), (what, st)
    COMPARED[0] += 1


def as_bytes(got):
    return got[0].tobytes() + got[1].tobytes() + got[2].tobytes()


def schedule(want, n, B, per_launch_pairs=None, chunk_rows=None):
    """The rounds (and kernel launches) of a call without seeds or cap, from its result: a round takes the first B rows of the list,
    those of them that are leaders are made, and every row one of the leaders made so far covers leaves the list."""
    leader_of = want[1].astype(np.int64)
    is_leader = np.zeros(n, bool)
    is_leader[want[0]] = True
    free = np.arange(n)
    made = rounds = 0
    launches = 1  # the first list
    while len(free):
        cand, rest = free[:B], free[B:]
        made += int(is_leader[cand].sum())
        launches += 2  # the resolve's two
        if len(rest):
            if per_launch_pairs is None:
                launches += 1
            else:
                per = max(per_launch_pairs // len(cand) // chunk_rows, 1) * chunk_rows
                launches += -(-len(rest) // per)
            launches += 1  # the compaction
        free = rest[leader_of[rest] >= made]
        rounds += 1
    return rounds, launches


WIDTHS = [128, 160, 256, 416, 512, 896, 1024, 2048, 4096]
KINDS = [O.KIND_SPARSE, O.KIND_DENSE, O.KIND_MORGAN]


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_oracle(bits, kind):
    W, n = bits // 32, 1203
    rng = np.random.default_rng(bits * 5 + kind)
    db, _ = planted(O.synth_rows(0x1EAD + bits + 13 * kind, kind, 0, n, W), rng)
    t = table(db)
    for kw in (TAN, TV):
        S = score_matrix(db, kw)
        compared = 0
        for cutoff in CUTOFFS:
            want = rule(S, cutoff)
            if not not_vacuous(want):
                continue
            what = (bits, kind, kw, cutoff)
            got = t.leader(cutoff, **kw)
            same(got, want, what)
            assert got[3]["rounds"] == schedule(want, n, DEFAULT_ROUND)[0], what
            only = t.leader(cutoff, assign=False, **kw)
            assert only[1] is None and only[2] is None
            same(only, want, what)
            compared += 1
        assert compared >= 1, ("every cutoff was vacuous", bits, kind, kw)
    print("leader calls compared with the oracle so far:", COMPARED[0])
    t.close()


def morgan_table(seed=0x1EADB, n=1203, W=32):
    rng = np.random.default_rng(seed)
    return planted(O.synth_rows(seed, O.KIND_MORGAN, 0, n, W), rng)


def test_the_result_does_not_depend_on_the_round_size():
    n, cutoff = 1203, 0.5
    db, _ = morgan_table()
    S = score_matrix(db)
    want = rule(S, cutoff)
    assert not_vacuous(want)
    L = len(want[0])
    first, rounds = None, {}
    for B in (1, 2, 7, 64, 256, 1024):
        t = table(db, round=B)
        got = t.leader(cutoff)
        same(got, want, ("round", B))
        first = first or as_bytes(got)
        assert as_bytes(got) == first, B
        rounds[B] = got[3]["rounds"]
        assert rounds[B] == schedule(want, n, B)[0], (B, rounds)
        if B == 1:  # the literal walk: one leader per round, and exactly the rule's scores
            assert rounds[B] == L and got[3]["pairs"] == want[3], (got[3], want[3])
        else:
            assert got[3]["pairs"] >= want[3] - B * L, "the resolve replaces at most B scores per leader"
        t.close()
    print("rounds by round size:", rounds)
    assert rounds[1] > rounds[7] > rounds[256] >= rounds[1024] and rounds[1024] <= 2


@pytest.mark.parametrize("bits", [128, 416, 2048])
def test_a_pass_cut_into_many_launches_gives_the_same_bytes(bits):
    n, W, cutoff = 2003, bits // 32, 0.5
    db, _ = morgan_table(0x1EADC + bits, n, W)
    chunk_rows = {128: 256, 416: 64, 2048: 64}[bits]
    nchunks = -(-(n - DEFAULT_ROUND) // chunk_rows)  # of the first pass
    want = rule(score_matrix(db), cutoff)
    assert not_vacuous(want)
    whole = table(db, pairs=1 << 40)
    a = whole.leader(cutoff)
    same(a, want, ("whole", bits))
    assert a[3]["launches"] == schedule(want, n, DEFAULT_ROUND)[1], a[3]
    for pairs, at_least in ((1, nchunks), (-(-nchunks // 5) * chunk_rows * DEFAULT_ROUND, 5 if nchunks >= 5 else nchunks)):
        cut = table(db, pairs=pairs)  # (a launch never covers less than one chunk of rows)
        b = cut.leader(cutoff)
        rounds, launches = schedule(want, n, DEFAULT_ROUND, pairs, chunk_rows)
        assert b[3]["launches"] == launches and b[3]["rounds"] == rounds == a[3]["rounds"], (b[3], launches)
        assert launches - a[3]["launches"] >= at_least - 1, "the first pass alone takes that many launches"
        assert as_bytes(b) == as_bytes(a), (bits, pairs)
        assert b[3]["pairs"] == a[3]["pairs"] and b[3]["assigned"] == n
        cut.close()
    if bits == 2048:
        assert nchunks >= 19
    assert 0 < a[3]["resolve_ms"] + a[3]["compact_ms"] < a[3]["kernel_ms"] and a[3]["wall_ms"] > 0
    whole.close()


def test_waves_that_take_several_chunks_of_a_launch():
    """The narrowest width on a table just large enough that, at the kernel's own geometry (twelve waves per compute unit, chunk c
    of a launch on wave c % nwaves), three quarters of the waves take two chunks of the first pass: the prefetched list entries of a
    second chunk, the counts carried from chunk to chunk.  Run in one launch, and cut at 0.65 x and 1.5 x the wave count in
    chunks.  Dense rows at a cutoff with few leaders keep the oracle cheap."""
    import torch
    W, cutoff, chunk_rows = 4, 0.3, 256
    nwaves = 12 * torch.cuda.get_device_properties(0).multi_processor_count
    n = nwaves * chunk_rows * 7 // 4 + DEFAULT_ROUND + 77
    db = O.synth_rows_mt(0x1EAD4, O.KIND_DENSE, 0, n, W)
    per = (n + NT - 1) // NT
    pool = ThreadPoolExecutor(NT)

    def score_row(r):
        out = np.empty(n, np.float32)
        list(pool.map(lambda lo: out.__setitem__(slice(lo, lo + per), O.tanimoto_raw(db[r], db[lo:lo + per])[0]), range(0, n, per)))
        return out

    want = leader_rule(score_row, n, cutoff, max_leaders=201)
    assert 5 <= len(want[0]) <= 200 and not (want[1] == NONE).any() and not_vacuous(want)
    assert -(-(n - DEFAULT_ROUND) // chunk_rows) > nwaves
    whole = table(db, pairs=1 << 40)
    a = whole.leader(cutoff)
    same(a, want, "several chunks per wave")
    assert a[3]["launches"] == schedule(want, n, DEFAULT_ROUND)[1]
    whole.close()
    for c in (nwaves * 13 // 20, nwaves * 3 // 2):
        pairs = c * chunk_rows * DEFAULT_ROUND
        cut = table(db, pairs=pairs)
        b = cut.leader(cutoff)
        assert b[3]["launches"] == schedule(want, n, DEFAULT_ROUND, pairs, chunk_rows)[1] > a[3]["launches"], (b[3], c)
        assert as_bytes(b) == as_bytes(a), c
        assert b[3]["pairs"] == a[3]["pairs"]
        cut.close()


def test_seeds():
    n, cutoff, base = 1203, 0.5, 5000
    db, block = morgan_table(0x1EAD5)
    S = score_matrix(db)
    t = table(db)
    cases = {
        "one seed covers the other": [block + 3, block + 1],  # identical rows: both leaders, the block joins the first
        "the last row": [n - 1],
        "five seeds": [700, 3, n - 1, block + 2, 41],
    }
    for what, seeds in cases.items():
        want = rule(S, cutoff, seeds)
        assert not_vacuous(want) and want[0][:len(seeds)].tolist() == seeds, what
        got = t.leader(cutoff, seeds=seeds)
        same(got, want, what)
    want = rule(S, cutoff, cases["one seed covers the other"])
    assert S[block + 3, block + 1] == 1.0 and want[1][block + 1] == 1 and want[1][block] == 0 and want[2][block] == 1.0
    t.close()
    two = table(db, round=2)  # several seed rounds, the last of them short
    want = rule(S, cutoff, cases["five seeds"])
    got = two.leader(cutoff, seeds=cases["five seeds"])
    same(got, want, "five seeds, two per round")
    two.close()
    based = table(db, base=base)
    seeds = [s + base for s in cases["five seeds"]]
    got = based.leader(cutoff, seeds=seeds)
    same(got, want, "seeds with a row base", base=base)
    with pytest.raises(capi.GsimError) as e:
        based.leader(cutoff, seeds=cases["five seeds"])  # without the base: outside the table
    assert e.value.code == -1
    based.close()


def test_the_cap():
    n, cutoff = 1203, 0.5
    db, _ = morgan_table(0x1EAD6)
    S = score_matrix(db)
    free = rule(S, cutoff)
    assert not_vacuous(free)
    L = len(free[0])
    t = table(db)
    for cap in (1, 100, L - 1, L, n):
        want = rule(S, cutoff, max_leaders=cap)
        got = t.leader(cutoff, max_leaders=cap)
        same(got, want, ("cap", cap))
        assert len(got[0]) == min(cap, L)
        unassigned = int(np.count_nonzero(got[1] == NONE))
        assert (unassigned > 0) == (cap < L), (cap, unassigned)
        assert not got[2][got[1] == NONE].any(), "an unassigned row scores 0.0"
        if cap >= L:
            assert as_bytes(got) == as_bytes(t.leader(cutoff))
    # cap = 100 falls in the middle of the first round's candidates: leader 100 is among the first 256 rows, and so are later ones
    assert free[0][99] < DEFAULT_ROUND - 1 and free[0][100] < DEFAULT_ROUND
    # ... and with seeds: a cap equal to their number
    seeds = [900, 5, 77]
    want = rule(S, cutoff, seeds, max_leaders=3)
    assert (want[1] == NONE).any()
    same(t.leader(cutoff, seeds=seeds, max_leaders=3), want, "seeds, nothing else")
    t.close()


def test_edges():
    W, cutoff = 32, 0.5
    some = O.synth_rows(0x1EAD7, O.KIND_MORGAN, 0, 300, W)
    # one row
    t = table(some[:1])
    leaders, leader_of, row_score, st = t.leader(cutoff)
    assert leaders.tolist() == [0] and leader_of.tolist() == [0] and row_score.tolist() == [1.0]
    assert st["leaders"] == st["assigned"] == st["rounds"] == 1 and st["pairs"] == 0
    t.close()
    # all rows identical: one leader
    t = table(np.repeat(some[:1], 300, 0))
    leaders, leader_of, row_score, st = t.leader(cutoff)
    assert leaders.tolist() == [0] and not leader_of.any() and (row_score == 1.0).all() and st["assigned"] == 300
    t.close()
    # all rows zero: every row a leader of a singleton; the second round has fewer than B candidates and an empty pass
    t = table(np.zeros((300, W), np.uint32))
    leaders, leader_of, row_score, st = t.leader(cutoff)
    assert np.array_equal(leaders, np.arange(300)) and np.array_equal(leader_of, np.arange(300)) and (row_score == 1.0).all()
    assert st["rounds"] == 2 and st["leaders"] == 300
    leaders, leader_of, row_score, st = t.leader(cutoff, max_leaders=10)
    assert np.array_equal(leaders, np.arange(10)) and (leader_of[10:] == NONE).all() and not row_score[10:].any()
    t.close()
    # cutoff 1.0: only duplicates join, zero rows never do
    db, block = morgan_table(0x1EAD8)
    n = len(db)
    S = score_matrix(db)
    want = rule(S, 1.0)
    assert not_vacuous(want)
    zero = np.flatnonzero(~db.any(1))
    assert len(zero) >= 3 and all(want[0][want[1][z]] == z for z in zero), "every zero row is its own leader"
    covered = np.flatnonzero(want[0][want[1]] != np.arange(n))
    assert len(covered) >= 40 and all((db[i] == db[want[0][want[1][i]]]).all() for i in covered), "only duplicates join"
    t = table(db)
    same(t.leader(1.0), want, "cutoff 1.0")
    # a cutoff equal to one pair's exact score: covered; the next f32 above it: not covered by that leader
    row0 = S[0].copy()
    row0[0] = 0
    row0[np.isnan(row0) | (row0 >= 1.0)] = 0
    j = int(np.argmax(row0))
    exact = float(row0[j])
    above = float(np.nextafter(np.float32(exact), np.float32(2)))
    assert 0 < exact < above < 1
    at, over = rule(S, exact), rule(S, above)
    assert at[1][j] == 0 and at[2][j] == np.float32(exact) and over[1][j] != 0
    same(t.leader(exact), at, "cutoff equal to a score")
    same(t.leader(above), over, "the next float above it")
    t.close()


def test_generated_and_attached_tables_row_base_and_the_search_state():
    import torch
    n, W, cutoff, base, seed = 2500, 32, 0.5, 7000, 0x1EAD9
    db = O.synth_rows(seed, O.KIND_MORGAN, 0, n, W)
    S = score_matrix(db, TV)
    want = rule(S, cutoff)
    assert not_vacuous(want)
    stored = table(db)
    singles = np.ascontiguousarray(db[[3, 1200, n - 1]])

    def searches():
        hits, approx = stored.search(singles, 50)
        return b"".join(h.tobytes() for h in hits) + approx.tobytes()

    before = searches()
    first = stored.leader(cutoff, **TV)
    same(first, want, "stored")
    assert searches() == before, "the search state is as it was"
    with pytest.raises(capi.GsimError):
        stored.leader(cutoff, max_leaders=n + 1)  # a failed call ...
    again = stored.leader(cutoff, **TV)  # ... and a correct one right after it
    assert as_bytes(again) == as_bytes(first), "the call repeated"
    assert searches() == before
    stored.close()
    generated = capi.Table(W * 32).generate(seed, O.KIND_MORGAN, 0, n, 0)
    same(generated.leader(cutoff, **TV), want, "generated")
    generated.set_row_base(base)
    same(generated.leader(cutoff, **TV), want, "generated, row base", base=base)
    generated.close()
    ten = torch.from_numpy(db.view(np.int32).copy()).to("cuda:0")
    attached = capi.Table(W * 32)
    attached.attach_device_rows(ten.data_ptr(), n, 0)
    got = attached.leader(cutoff, **TV)
    same(got, want, "attached")
    assert as_bytes(got) == as_bytes(first)
    attached.close()
    del ten
