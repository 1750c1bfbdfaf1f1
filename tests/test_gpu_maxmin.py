"""gsim_db_maxmin on the GPU: picks, pick scores, row scores and nearest picks against the pinned per-row scores of oracle_lib
fed through the numpy restatement of the rule (maxmin_rule.py) -- picks and nearest exactly, scores bit for bit -- over the
widths and table kinds of the scan, the edge cases of the rule, multi-launch passes, and property checks at 100 M rows."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as O
from gpusimilarity_amd import capi
from gpusimilarity_amd.fingerprintdb import FingerprintDB
from maxmin_rule import maxmin_rule

pytestmark = pytest.mark.gpu
NT = 16
TV = dict(metric=capi.METRIC_TVERSKY, alpha=0.5, beta=0.5)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def table(db, device=0):
    return capi.Table(db.shape[1] * 32).add_rows(db).finalize(device, 1)


def tanimoto_rows(db):
    """score(query = row r, every row): oracle_lib.tanimoto_raw on NT host threads."""
    n = db.shape[0]
    per = max(1, (n + NT - 1) // NT)
    pool = ThreadPoolExecutor(NT)

    def score_row(r):
        out = np.empty(n, np.float32)

        def part(lo):
            out[lo:lo + per] = O.tanimoto_raw(db[r], db[lo:lo + per])[0]
        list(pool.map(part, range(0, n, per)))
        return out
    return score_row


def tversky_rows(db, alpha, beta):
    """... Tversky: oracle_lib.search(row r, table, k = N, cutoff = 0) -- every row, a NaN score reported as 0."""
    n = db.shape[0]

    def score_row(r):
        hits, _ = O.search(db[r], db, n, 0.0, O.METRIC_TVERSKY, alpha, beta, nthreads=NT)
        out = np.zeros(n, np.float32)
        out[hits["row"]] = hits["score"]
        return out
    return score_row


def oracle(db, npicks, seeds=(), max_score=1.0, metric=capi.METRIC_TANIMOTO, alpha=1.0, beta=1.0):
    f = tanimoto_rows(db) if metric == capi.METRIC_TANIMOTO else tversky_rows(db, alpha, beta)
    return maxmin_rule(f, db.shape[0], npicks, seeds, max_score)


def same(got, want, row_base=0):
    gp, gs, grs, gn = got
    wp, ws, wrs, wn = want
    assert np.array_equal(gp, wp + np.uint32(row_base)), (gp[:20], wp[:20])
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32))
    assert np.array_equal(grs.view(np.uint32), wrs.view(np.uint32))
    assert np.array_equal(gn, wn)


def special_rows(db, rng):
    """duplicates (maxsim 1.0 ties), all-zero rows (NaN), a block of identical rows (the tie-break decides)"""
    n = db.shape[0]
    for i in rng.choice(n, 6, replace=False):
        db[int(rng.integers(n))] = db[i]
    db[rng.choice(n, 3, replace=False)] = 0
    b = int(rng.integers(0, n - 40))
    db[b:b + 40] = db[b]
    return db


WIDTHS = [128, 160, 192, 256, 512, 896, 1024, 2048, 4096]
KINDS = [O.KIND_SPARSE, O.KIND_DENSE, O.KIND_MORGAN]


@pytest.mark.parametrize("bits", WIDTHS + [64, 416])
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_oracle(bits, kind):
    W = bits // 32
    n = 3000 if kind != O.KIND_DENSE else 2000
    rng = np.random.default_rng(bits * 7 + kind)
    db = special_rows(O.synth_rows(0x3A11 + bits + 11 * kind, kind, 0, n, W), rng)
    t = table(db)
    for kw, npicks in ((dict(), 120), (TV, 60)):
        got = t.maxmin(npicks, assign=True, **kw)
        same(got, oracle(db, npicks, **kw))
    t.close()


def test_parity_on_a_larger_table_with_seeds():
    n, W = 20000, 32
    rng = np.random.default_rng(5)
    db = special_rows(O.synth_rows(0x3A12, O.KIND_MORGAN, 0, n, W), rng)
    t = table(db)
    seeds = [17, 19999, 4242]
    same(t.maxmin(300, seeds=seeds, assign=True), oracle(db, 300, seeds))
    same(t.maxmin(300, seeds=seeds, assign=True, **TV), oracle(db, 300, seeds, **TV))
    t.close()


def test_edge_cases():
    W = 32
    db = O.synth_rows(0x3A13, O.KIND_SPARSE, 0, 700, W)
    db[100:110] = db[3]
    t = table(db)
    # npicks == N: a permutation of the rows (duplicates of picks are picked, in their turn)
    got = t.maxmin(700, assign=True)
    same(got, oracle(db, 700))
    assert sorted(got[0].tolist()) == list(range(700))
    # npicks == 0
    p, s = t.maxmin(0)
    assert len(p) == 0 and len(s) == 0
    # nseeds == npicks, seeds only
    same(t.maxmin(3, seeds=[5, 600, 9], assign=True), oracle(db, 3, [5, 600, 9]))
    same(t.maxmin(1, seeds=[42], assign=True), oracle(db, 1, [42]))
    # an early stop; *npicked
    full = oracle(db, 400)
    ms = float(np.nextafter(full[1][200], np.float32(0)))  # just under pick 200's score
    want = oracle(db, 400, max_score=ms)
    assert 1 < len(want[0]) <= 200
    st = {}
    got = t.maxmin(400, max_score=ms, assign=True, stats=st)
    same(got, want)
    assert st["picks"] == len(want[0])
    # max_score 0: only the seeds
    same(t.maxmin(50, seeds=[7, 8], max_score=0.0, assign=True), oracle(db, 50, [7, 8], max_score=0.0))
    # without assign: the same picks
    p, s = t.maxmin(200)
    w = oracle(db, 200)
    assert np.array_equal(p, w[0]) and np.array_equal(s.view(np.uint32), w[1].view(np.uint32))
    t.close()
    # N = 1, N = 2
    for n in (1, 2):
        d = O.synth_rows(0x3A14, O.KIND_DENSE, 0, n, W)
        tt = table(d)
        for npk in range(n + 1):
            if npk:
                same(tt.maxmin(npk, assign=True), oracle(d, npk))
        tt.close()
    z = table(np.zeros((2, W), np.uint32))  # two all-zero rows: 0/0 = NaN counts as 0
    same(z.maxmin(2, assign=True), oracle(np.zeros((2, W), np.uint32), 2))
    z.close()


def test_row_base():
    W = 16
    db = O.synth_rows(0x3A15, O.KIND_MORGAN, 0, 2500, W)
    t = table(db)
    t.set_row_base(1000)
    got = t.maxmin(80, seeds=[1000 + 77, 1000 + 2499], assign=True)
    same(got, oracle(db, 80, [77, 2499]), row_base=1000)
    with pytest.raises(capi.GsimError) as e:
        t.maxmin(5, seeds=[77])  # a seed below the row base
    assert e.value.code == -1
    t.close()


def test_determinism_and_the_rest_of_the_handle():
    n, W = 30000, 32
    db = O.synth_rows(0x3A16, O.KIND_MORGAN, 0, n, W)
    t = table(db)
    qs = db[[O.query_row(i, n) for i in range(4)]]
    before = t.search(qs, 50)
    a = t.maxmin(150, assign=True)
    b = t.maxmin(150, assign=True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    after = t.search(qs, 50)
    for h0, h1 in zip(before[0], after[0]):
        assert h0.tobytes() == h1.tobytes()
    assert np.array_equal(before[1], after[1])
    t.close()


def test_multi_launch_passes_give_the_same_result(tmp_path):
    """Test-hooks build, GSIM_TEST_MAXMIN_LAUNCH_ROWS = 16384: every pass over 50 000 rows runs in 4 launches."""
    from conftest import hooks_env, HOOKS_LIB
    assert os.path.exists(HOOKS_LIB)
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import numpy as np, oracle_lib as O; from gpusimilarity_amd import capi\n"
            "out = {}\n"
            "for bits in (1024, 160, 896):\n"
            "    db = O.synth_rows(0x3A17 + bits, O.KIND_MORGAN, 0, 50000, bits // 32)\n"
            "    t = capi.Table(bits).add_rows(db).finalize(0, 1)\n"
            "    st = {}\n"
            "    r = t.maxmin(120, seeds=[3, 49999], assign=True, stats=st)\n"
            "    t.close()\n"
            "    out.update({'%%d_%%d' %% (bits, i): x for i, x in enumerate(r)})\n"
            "    out['%%d_launches' %% bits] = np.array(st['launches'])\n"
            "np.savez(sys.argv[1], **out)\n"
            % (ROOT, os.path.join(ROOT, "tests")))
    runs = {}
    for cap in ("16384", None):
        env = hooks_env(GSIM_TEST_MAXMIN_LAUNCH_ROWS=cap) if cap else hooks_env()
        path = str(tmp_path / ("run_%s.npz" % cap))
        r = subprocess.run([sys.executable, "-c", code, path], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        runs[cap] = np.load(path)
    capped, whole = runs["16384"], runs[None]
    for bits in (1024, 160, 896):
        # the last pick's pass is run too (assign): 120 passes
        assert int(whole["%d_launches" % bits]) == 120 and int(capped["%d_launches" % bits]) == 4 * 120, bits
        for i in range(4):
            k = "%d_%d" % (bits, i)
            assert capped[k].tobytes() == whole[k].tobytes(), k


def test_fingerprintdb_maxmin():
    n, W = 4000, 32
    db = O.synth_rows(0x3A18, O.KIND_MORGAN, 0, n, W)
    fdb = FingerprintDB(1024, n, "k", [db], [b"s%d" % i for i in range(n)], [b"i%d" % i for i in range(n)])
    fdb.copyToGPU()
    want = oracle(db, 60)
    picks = fdb.maxmin(60)
    assert picks == want[0].tolist()
    picks2, clusters = fdb.maxmin(60, assign=True)
    assert picks2 == picks and len(clusters) == 60
    assert sorted(r for c in clusters for r in c) == list(range(n))
    for j, c in enumerate(clusters):
        assert c[0] == picks[j] and all(want[3][r] == j for r in c)


def test_one_million_morgan_rows():
    n, W, npicks = 1_000_000, 32, 1000
    db = O.synth_rows_mt(0x3A19, O.KIND_MORGAN, 0, n, W, nthreads=NT)
    t = table(db)
    st = {}
    got = t.maxmin(npicks, seeds=[12345], assign=True, stats=st)
    assert st["picks"] == npicks and st["launches"] == npicks
    same(got, oracle(db, npicks, [12345]))
    t.close()


def test_one_hundred_million_rows_properties():
    n, bits, npicks, seed = 100_000_000, 1024, 200, 0x3A1A
    W = bits // 32
    t = capi.Table(bits).generate(seed, capi.SYNTH_SPARSE, 0, n, 0)
    st = {}
    picks, ps, rs, nr = t.maxmin(npicks, assign=True, stats=st)
    t.close()
    assert len(picks) == npicks and len(set(picks.tolist())) == npicks
    prow = np.stack([capi.synth_row(seed, capi.SYNTH_SPARSE, int(r), bits) for r in picks])
    # pick_scores: each pick's largest score against the picks before it, recomputed from the picked rows
    sc = np.stack([O.tanimoto_raw(prow[j], prow)[0] for j in range(npicks)])
    sc = np.where(np.isnan(sc), np.float32(0), sc)
    want_ps = np.array([0.0] + [sc[:j, j].max() for j in range(1, npicks)], np.float32)
    assert np.array_equal(ps.view(np.uint32), want_ps.view(np.uint32))
    assert (np.diff(ps[1:]) >= 0).all()
    unpicked = np.ones(n, bool)
    unpicked[picks] = False
    assert (rs[unpicked] >= ps[-1]).all()
    assert (rs[~unpicked] == 1.0).all() and (nr[picks] == np.arange(npicks)).all()
    # 10 000 sampled rows, regenerated on the host: row_score and nearest against the picked rows
    rows = np.random.default_rng(3).choice(n, 10_000, replace=False)
    samp = np.stack([capi.synth_row(seed, capi.SYNTH_SPARSE, int(r), bits) for r in rows])
    s = np.stack([O.tanimoto_raw(prow[j], samp)[0] for j in range(npicks)])
    s = np.where(np.isnan(s), np.float32(0), s)
    best = s.max(axis=0)
    first = s.argmax(axis=0)  # the earliest pick attaining the maximum
    up = unpicked[rows]
    assert np.array_equal(rs[rows][up].view(np.uint32), best[up].view(np.uint32))
    assert np.array_equal(nr[rows][up], first[up].astype(np.uint32))
