"""Group queries on the GPU (gsim_db_search_group): exact top-k by the MAX, MIN or MEAN of a row's scores against a set of queries.

Expected values: the oracle gives the pair scores -- oracle_lib.search(q, db, k=n, cutoff=0.0, ...) returns all n rows with NaN
already 0, scattered back by row -- the group rule of include/gpusim_hip.h is applied to them in numpy f32 (MEAN: the sequential
loop, query 0 first), and the ordering is oracle_lib.canonical_topk_from_scores'.  Rows, score bits, `which`, popc_db, count and
approx are compared.  Everything is exact: no tolerances."""
import contextlib
import os

import numpy as np
import pytest

import oracle_lib as O
from gpusimilarity_amd import capi

pytestmark = pytest.mark.gpu
NT = 16
KNOB = "GSIM_GROUP_LAUNCH_PAIRS"
MAX, MIN, MEAN = capi.GROUP_MAX, capi.GROUP_MIN, capi.GROUP_MEAN
MODES = [MAX, MIN, MEAN]
TAN = dict()
TV37 = dict(metric=capi.METRIC_TVERSKY, alpha=0.3, beta=0.7)
SCREEN = dict(metric=capi.METRIC_TVERSKY, alpha=1.0, beta=0.0)
METRICS = [TAN, TV37, SCREEN]
COMPARED = [0]  # group queries compared with the oracle so far (printed by every test that adds to it)


@contextlib.contextmanager
def knob(value):
    """The launch knob is read once per handle, by gsim_db_create: set it around the creation of a table."""
    old = os.environ.get(KNOB)
    if value is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = old


def table(db, pairs=None, base=0):
    with knob(pairs):
        t = capi.Table(db.shape[1] * 32).add_rows(db).finalize(0, 1)
    if base:
        t.set_row_base(base)
    return t


def popc_rows(db):
    return np.unpackbits(np.ascontiguousarray(db).view(np.uint8), axis=1).sum(1).astype(np.uint16)


def pair_scores(queries, db, kw):
    """S[i, r] = the score gsim_db_search returns for query i and row r at cutoff 0 (NaN already 0), from the oracle."""
    n = len(db)
    S = np.empty((len(queries), n), np.float32)
    for i, q in enumerate(queries):
        hits, approx = O.search(q, db, n, 0.0, kw.get("metric", 0), kw.get("alpha", 1.0), kw.get("beta", 1.0), nthreads=NT)
        assert len(hits) == n and approx == n
        S[i, hits["row"]] = hits["score"]
    assert not np.isnan(S).any() and S.min() >= 0 and S.max() <= 1
    return S


def mean_in_order(S):
    acc = np.zeros(S.shape[1], np.float32)
    for i in range(S.shape[0]):
        acc = (acc + S[i]).astype(np.float32)  # one IEEE f32 rounding per step, query order
    return (acc / np.float32(S.shape[0])).astype(np.float32)


def group_scores(S, mode):
    if mode == MAX:
        return S.max(0), S.argmax(0)  # (argmax / argmin: the first, i.e. lowest, index that attains it)
    if mode == MIN:
        return S.min(0), S.argmin(0)
    return mean_in_order(S), np.zeros(S.shape[1], np.int64)


def expected(S, mode, k, cutoff, popc, base=0):
    g, which = group_scores(S, mode)
    rows, s, approx = O.canonical_topk_from_scores(g, k, cutoff)
    want = np.zeros(len(rows), capi.GROUP_HIT_DTYPE)
    want["row"] = rows + base
    want["score"] = s
    want["which"] = which[rows]
    want["popc_db"] = popc[rows]
    return want, approx


def same(got, approx, want, wap, what):
    assert len(got) == len(want), what
    assert np.array_equal(got["row"], want["row"]), what
    assert np.array_equal(got["score"].view(np.uint32), want["score"].view(np.uint32)), what
    assert np.array_equal(got["which"], want["which"]), what
    assert np.array_equal(got["popc_db"], want["popc_db"]), what
    assert int(approx) == wap, what
    COMPARED[0] += 1


def check(t, queries, S, mode, k, cutoff, kw, popc, what, base=0, empty=False):
    hits, approx = t.search_group(queries, k, mode, cutoff, **kw)
    want, wap = expected(S, mode, k, cutoff, popc, base)
    if empty:
        assert len(want) == 0 and wap == 0, what
    elif k:
        assert len(want) > 0, ("a vacuous case", what)
    same(hits, approx, want, wap, what)
    return hits.tobytes() + np.uint64(approx).tobytes()


WIDTHS = [128, 160, 256, 416, 512, 896, 1024, 2048, 4096]
KINDS = [O.KIND_SPARSE, O.KIND_DENSE, O.KIND_MORGAN]


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_oracle(bits, kind):
    W = bits // 32
    n = 1203
    assert all(n % c >= 3 for c in (8, 16, 32, 64, 128, 256, 512)), "the last chunk is partial for every chunk size"
    db = O.synth_rows(0x6A0 + bits + 7 * kind, kind, 0, n, W)
    db[n // 2] = 0  # an all-zero row
    rng = np.random.default_rng(bits * 3 + kind)
    # table rows plus one random fingerprint (query 1): every M below takes the first M of these
    queries = db[rng.choice(n, 64, replace=False)].copy()
    queries[1] = rng.integers(0, 2**32, W, dtype=np.uint32) & rng.integers(0, 2**32, W, dtype=np.uint32)
    popc = popc_rows(db)
    t = table(db)
    for kw in METRICS:
        S64 = pair_scores(queries, db, kw)
        for M in (1, 2, 3, 17, 64):
            S = S64[:M]
            for mode in MODES:
                g = group_scores(S, mode)[0]
                ranked = np.sort(g)[::-1]
                mid = float(np.float32((float(ranked[0]) + float(ranked[n // 2])) / 2))
                at_rank_50 = float(ranked[49])  # exactly the 50th row's group score: the boundary is inclusive
                for cutoff in (0.0, mid, at_rank_50):
                    if cutoff > 0:
                        assert np.count_nonzero(g >= np.float32(cutoff)) >= (50 if cutoff == at_rank_50 else 1)
                    for k in (1, 100, n, n + 5):
                        check(t, queries[:M], S, mode, k, cutoff, kw, popc, (bits, kind, kw, M, mode, k, cutoff))
    for mode in MODES:  # nq = 1 is gsim_db_search's result, with which = 0
        one, oap = t.search_group(queries[:1], 100, mode)
        ref, rap = t.search(queries[0], 100)
        assert np.array_equal(one["row"], ref[0]["row"]) and np.array_equal(one["score"].view(np.uint32), ref[0]["score"].view(np.uint32))
        assert np.array_equal(one["popc_db"], ref[0]["popc_db"]) and not one["which"].any() and oap == int(rap[0])
    none, nap = t.search_group(queries[:3], 0, MEAN)  # k = 0 is legal
    assert none.size == 0 and nap == n
    print("group queries compared with the oracle so far:", COMPARED[0])
    t.close()


@pytest.mark.parametrize("W", [4, 32])
@pytest.mark.parametrize("kind", KINDS)
def test_mean_sums_in_query_order(W, kind):
    n = 1203
    db = O.synth_rows(0x6A0 + W + kind, kind, 0, n, W)
    popc = popc_rows(db)
    t = table(db)
    for M in (3, 7, 17):
        queries = db[[(53 * i) % n for i in range(M)]]
        S = pair_scores(queries, db, TAN)
        want, wap = expected(S, MEAN, 100, 0.0, popc)
        rows = want["row"].astype(np.int64)
        forward, backward = mean_in_order(S)[rows], mean_in_order(S[::-1])[rows]
        differ = int(np.count_nonzero(forward.view(np.uint32) != backward.view(np.uint32)))
        print("W", W, "kind", kind, "M", M, "top-100 rows whose mean depends on the order:", differ)
        assert differ >= 10, "the shape does not tell the orders apart"
        hits, approx = t.search_group(queries, 100, MEAN)
        same(hits, approx, want, wap, (W, kind, M))
    t.close()


def test_max_against_the_merged_single_query_lists():
    """No oracle: MAX's hits are the M gsim_db_search top-k lists merged -- per row the largest score, then (score desc, row asc)."""
    n, W, k, M = 20011, 32, 100, 17
    db = O.synth_rows(0x6A17, O.KIND_MORGAN, 0, n, W)
    queries = db[[(1009 * i + 5) % n for i in range(M)]]
    t = table(db)
    lists, _ = t.search(queries, k)
    best = {}
    for h in lists:
        assert len(h) == k
        for row, score in zip(h["row"].tolist(), h["score"].tolist()):
            best[row] = max(best.get(row, 0.0), score)
    merged = sorted(best.items(), key=lambda rs: (-rs[1], rs[0]))[:k]
    hits, approx = t.search_group(queries, k, MAX)
    assert len(hits) == k and approx == n
    assert hits["row"].tolist() == [r for r, _ in merged]
    assert np.array_equal(hits["score"].view(np.uint32), np.array([s for _, s in merged], np.float32).view(np.uint32))
    t.close()


def test_ties_keep_the_lowest_rows_and_the_lowest_query():
    n, W = 1203, 32
    db = O.synth_rows(0x6A71E, O.KIND_MORGAN, 0, n, W)
    rng = np.random.default_rng(71)
    copies = np.sort(rng.choice(n, 300, replace=False))
    db[copies] = db[copies[0]]
    strangers = O.synth_rows(0x6A71E, O.KIND_MORGAN, n, 3, W)  # (not rows of the table: nothing else scores 1.0)
    queries = np.stack([strangers[0], strangers[1], db[copies[5]], strangers[2], db[copies[9]]])  # queries 2 and 4 are identical: the tied row
    assert not (db[:, None, :] == strangers[None]).all(2).any()
    t = table(db)
    hits, approx = t.search_group(queries, 100, MAX)
    assert len(hits) == 100 and approx == n
    assert np.array_equal(hits["row"], copies[:100]), "the 100 lowest-numbered copies"
    assert (hits["score"] == 1.0).all() and (hits["which"] == 2).all(), "the lower of the two identical queries"
    S = pair_scores(queries, db, TAN)
    check(t, queries, S, MAX, 100, 0.0, TAN, popc_rows(db), "ties")
    check(t, queries, S, MAX, 350, 1.0, TAN, popc_rows(db), "ties, cutoff 1.0")
    t.close()


@pytest.mark.parametrize("n", [1203, 20011])
def test_an_all_zero_query_in_the_set(n):
    """MIN is 0 everywhere.  n = 20011: more rows tie in bin 0 than the select kernel ranks in LDS -- its heavy-tie path rebuilds
    the hits, and `which` comes from the kernel behind it."""
    W, k = 4, 100
    db = O.synth_rows(0x6A00 + n, O.KIND_SPARSE, 0, n, W)
    queries = np.concatenate([db[[11, 500]], np.zeros((1, W), np.uint32), db[[900]]])
    popc = popc_rows(db)
    S = pair_scores(queries, db, TAN)
    assert (S[2] == 0).all()
    t = table(db)
    check(t, queries, S, MIN, k, 0.25, TAN, popc, "empty: MIN under a cutoff", empty=True)
    hits, approx = t.search_group(queries, k, MIN)
    assert np.array_equal(hits["row"], np.arange(k)) and (hits["score"] == 0).all() and approx == n
    for mode in MODES:  # (MAX ignores the zero query, MEAN divides by 4)
        check(t, queries, S, mode, k, 0.0, TAN, popc, ("zeros", mode))
    check(t, queries, S, MAX, k, 0.3, TAN, popc, "zeros, MAX, cutoff")
    check(t, queries, S, MEAN, k, 0.05, TAN, popc, "zeros, MEAN, cutoff")
    print("group queries compared with the oracle so far:", COMPARED[0])
    t.close()


def test_the_largest_query_set():
    n, W, M = 300, 4, 1024
    db = O.synth_rows(0x6A1024, O.KIND_DENSE, 0, n, W)
    rng = np.random.default_rng(1024)
    queries = rng.integers(0, 2**32, (M, W), dtype=np.uint32)
    queries[1023] = db[7]
    assert not (queries[:1023] == db[7]).all(1).any(), "query 1023 alone equals row 7"
    popc = popc_rows(db)
    S = pair_scores(queries, db, TAN)
    t = table(db)
    hits, approx = t.search_group(queries, 10, MAX)
    assert hits[0]["row"] == 7 and hits[0]["score"] == 1.0 and hits[0]["which"] == 1023
    for mode in MODES:
        check(t, queries, S, mode, 50, 0.0, TAN, popc, ("M = 1024", mode))
    with pytest.raises(capi.GsimError) as e:
        t.search_group(np.concatenate([queries, queries[:1]]), 10, MAX)
    assert e.value.code == -1
    t.close()


@pytest.mark.parametrize("mode", [MAX, MEAN])
def test_k_above_the_select_kernels_capacity(mode):
    n, W, k, M = 20011, 4, 9000, 5
    assert k > capi.SELECT_CAP
    db = O.synth_rows(0x6A9000, O.KIND_MORGAN, 0, n, W)
    queries = db[[(4001 * i + 17) % n for i in range(M)]]
    S = pair_scores(queries, db, TAN)
    t = table(db)
    check(t, queries, S, mode, k, 0.0, TAN, popc_rows(db), ("large k", mode))
    t.close()


@pytest.mark.parametrize("bits", [128, 416, 1024])
def test_a_pass_cut_into_many_launches_gives_the_same_bytes(bits):
    n, W, M = 1203, bits // 32, 17
    db = O.synth_rows(0x6AC07 + bits, O.KIND_MORGAN, 0, n, W)
    queries = db[[(53 * i) % n for i in range(M)]]
    whole, cut = table(db), table(db, pairs="1")  # (a launch never covers less than one chunk of rows)
    S = pair_scores(queries, db, TAN)
    for mode in MODES:
        at_rank_50 = float(np.sort(group_scores(S, mode)[0])[::-1][49])
        for k, cutoff in ((100, 0.0), (n, 0.0), (100, at_rank_50)):
            a, aap, ast = whole.search_group(queries, k, mode, cutoff, stats=True)
            b, bap, bst = cut.search_group(queries, k, mode, cutoff, stats=True)
            assert len(a) > 0
            tail = 3  # compaction, select, `which`
            assert ast["launches"] == 1 + tail and bst["launches"] >= 5 + tail, (ast, bst)
            assert ast["queries"] == M == bst["queries"] and ast["pairs"] == n * M == bst["pairs"]
            assert 0 < ast["scan_ms"] <= ast["kernel_ms"] and ast["wall_ms"] > 0
            assert a.tobytes() == b.tobytes() and aap == bap, (bits, mode, k, cutoff)
    check(cut, queries, S, MEAN, 100, 0.0, TAN, popc_rows(db), "cut, against the oracle")
    whole.close()
    cut.close()


@pytest.mark.parametrize("bits, n", [(128, 1600003), (160, 400003)])
def test_waves_that_take_several_chunks_over_several_launches(bits, n):
    """More chunks than waves -- what a table large enough to need launch cutting looks like.  The grid is twelve waves per compute
    unit and chunk c belongs to wave c % nwaves, so with more than two chunks per wave a wave loops inside a launch (the threshold
    poll sees a second trip) and, where a launch covers fewer chunks than there are waves, appends behind the cursor its own
    earlier chunk left in seg_count (a non-zero start into its segment).  128-bit rows: 256-row chunks, the register kernel;
    160-bit rows: 64-row chunks, the word loop.  Two cuts: 0.65 x nwaves chunks per launch (no wave loops inside a launch, the
    launches' first chunks fall on changing waves) and 1.5 x nwaves (some waves take two chunks of a launch, some one).  Every
    result is compared with the oracle and, for the cut handles, with the uncut handle's bytes; two of the three cases have a cutoff,
    so `approx` checks the launches' increments to `kept`."""
    import torch
    W, M = bits // 32, 3
    chunk_rows = 256 if bits == 128 else 64
    nwaves = 12 * torch.cuda.get_device_properties(0).multi_processor_count
    nchunks = -(-n // chunk_rows)
    assert nchunks > 2 * nwaves and n % chunk_rows, "every wave takes at least two chunks, the last chunk is partial"
    db = O.synth_rows(0x6AB16 + bits, O.KIND_MORGAN, 0, n, W)
    queries = db[[(100003 * i + 11) % n for i in range(M)]]
    popc = np.bitwise_count(db).sum(1).astype(np.uint16)
    S = pair_scores(queries, db, TAN)
    per_launch = [nwaves * 13 // 20, nwaves * 3 // 2]
    whole = table(db, pairs=str(1 << 40))
    cuts = [table(db, pairs=str(c * chunk_rows * M)) for c in per_launch]
    for mode in MODES:
        ranked = np.sort(group_scores(S, mode)[0])[::-1]
        assert ranked[20000] > 0, "the cutoffs below are cutoffs"
        for k, cutoff in ((100, 0.0), (5000, float(ranked[20000])), (100, float(ranked[49]))):
            what = (bits, mode, k, cutoff)
            a, aap, ast = whole.search_group(queries, k, mode, cutoff, stats=True)
            want, wap = expected(S, mode, k, cutoff, popc)
            assert len(want) == min(k, wap) and (50 <= wap < n if cutoff else wap == n), what
            same(a, aap, want, wap, what)
            assert ast["launches"] == 1 + 3 and ast["pairs"] == n * M, ast
            for t, c in zip(cuts, per_launch):
                b, bap, bst = t.search_group(queries, k, mode, cutoff, stats=True)
                assert bst["launches"] == -(-nchunks // c) + 3 and bst["launches"] >= 2 + 3, (bst, c)
                assert b.tobytes() == a.tobytes() and bap == aap, (what, c)
    print("group queries compared with the oracle so far:", COMPARED[0])
    for t in [whole] + cuts:
        t.close()


def test_the_search_state_is_left_as_it_was_found():
    n, W, k = 20011, 32, 50
    db = O.synth_rows(0x6A57A7E, O.KIND_MORGAN, 0, n, W)
    singles = np.ascontiguousarray(db[[3, 4000, 19999]])
    group = db[[(1009 * i + 5) % n for i in range(7)]]
    counters = ("handed_back", "handed_back_why", "rerun_own", "rerun_publish", "rerun_behind", "rerun_torn", "lane_queries", "backoff_skips")
    t = table(db)
    t.enable_timing(True)

    def searches():
        hits, approx = t.search(singles, k)
        bufs = t.make_search_buffers(len(singles), k)
        t.search_each_into(singles, k, bufs)
        return b"".join(h.tobytes() for h in hits) + approx.tobytes() + b"".join(x.tobytes() for x in bufs)

    before = searches()
    tm = t.timing()
    first = t.search_group(group, k, MEAN)
    assert {c: t.timing()[c] for c in counters} == {c: tm[c] for c in counters}
    assert searches() == before
    with pytest.raises(capi.GsimError):
        t.search_group(group, k, 9)  # a failed call ...
    again = t.search_group(group, k, MEAN)  # ... and a correct one right after it
    assert again[0].tobytes() == first[0].tobytes() and again[1] == first[1]
    check(t, group, pair_scores(group, db, TAN), MEAN, k, 0.0, TAN, popc_rows(db), "after a failed call")
    assert searches() == before
    t.close()


def test_row_base_generated_and_attached_tables():
    import torch
    n, W, M, base = 2500, 32, 6, 5000
    seed = 0x6A77
    db = O.synth_rows(seed, O.KIND_MORGAN, 0, n, W)
    queries = db[[(419 * i + 3) % n for i in range(M)]]
    popc = popc_rows(db)
    S = pair_scores(queries, db, TV37)
    based = table(db, base=base)
    generated = capi.Table(W * 32).generate(seed, O.KIND_MORGAN, 0, n, 0)
    ten = torch.from_numpy(db.view(np.int32).copy()).to("cuda:0")
    attached = capi.Table(W * 32)
    attached.attach_device_rows(ten.data_ptr(), n, 0)
    for mode in MODES:
        check(based, queries, S, mode, 100, 0.1, TV37, popc, ("row base", mode), base=base)
        check(generated, queries, S, mode, 100, 0.1, TV37, popc, ("generated", mode))
        check(attached, queries, S, mode, 100, 0.1, TV37, popc, ("attached", mode))
    for t in (based, generated, attached):
        t.close()
    del ten


def test_the_same_call_twice_gives_identical_bytes():
    n, W, M = 20011, 8, 33
    db = O.synth_rows(0x6A2, O.KIND_DENSE, 0, n, W)
    queries = db[[(701 * i) % n for i in range(M)]]
    t = table(db)
    for mode in MODES:
        for k, cutoff in ((1000, 0.0), (1000, 0.3)):
            a = t.search_group(queries, k, mode, cutoff, **TV37)
            b = t.search_group(queries, k, mode, cutoff, **TV37)
            assert len(a[0]) > 0 and a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    t.close()
