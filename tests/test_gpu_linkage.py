"""Complete- and average-linkage dendrograms on the GPU (gsim_db_linkage).

Expected values: the oracle gives the pair scores (test_gpu_components.score_matrix; 0 / 0 is 0.0f) and linkage_rule.greedy -- the
definition of include/gpusim_hip.h's rule -- is applied to them; linkage_rule.chain gives the scans and the chain's depth.  Every
comparison is on bytes: no tolerances.  The planted table of 2500 rows (two full strides of the chain kernel's 1024 threads and a
partial one) has 1500 identical rows, a 250-row sliding-window chain, near-copies and zero rows, so the expected dendrograms tie
heavily; `not_vacuous` asserts that on the expected result."""
import os
import subprocess
import sys

import numpy as np
import pytest

import linkage_rule as R
import oracle_lib as O
from gpusimilarity_amd import capi
from test_gpu_components import TV, planted_table, score_matrix, table

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2500
KINDS = (capi.LINKAGE_COMPLETE, capi.LINKAGE_AVERAGE)
_WANT = {}


def scores_of(bits):
    db, _, S = planted_table(bits, N)
    key = ("S", bits)
    if key not in _WANT:
        Z = np.where(np.isnan(S), np.float32(0), S)  # 0 / 0 is 0.0f
        Z.setflags(write=False)
        _WANT[key] = Z
    return db, _WANT[key]


def expected(bits, kind):
    """(merges, scans, chain_max) of the planted table of that width: computed once, never changed"""
    if (bits, kind) not in _WANT:
        _, S = scores_of(bits)
        want = R.greedy(S, kind)
        via_chain, scans, chain_max = R.chain(S, kind)
        assert via_chain.tobytes() == want.tobytes()
        want.setflags(write=False)
        _WANT[(bits, kind)] = (want, scans, chain_max)
    return _WANT[(bits, kind)]


def not_vacuous(want, scans, chain_max, n):
    score, counts = np.unique(want["score"], return_counts=True)
    return int(counts[counts > 1].sum()) >= 1000 and len(score) >= 20 and chain_max >= 3 and scans > n


def same(got, st, want, scans, chain_max, what, offset=0):
    shifted = want.copy()
    shifted["a"] += np.uint32(offset)
    shifted["b"] += np.uint32(offset)
    assert got.dtype == capi.LINKAGE_MERGE_DTYPE and got.tobytes() == shifted.tobytes(), (what, got[:5], shifted[:5])
    n = len(want) + 1
    assert (st["rows"], st["merges"], st["scans"], st["chain_max"]) == (n, n - 1, scans, chain_max), (what, st, scans, chain_max)
    assert st["launches"] == -(-scans // st["launch_steps"]), (what, st)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bits", [128, 160, 1024, 4096])
def test_parity_with_the_rule(bits, kind):
    db, _ = scores_of(bits)
    want, scans, chain_max = expected(bits, kind)
    assert not_vacuous(want, scans, chain_max, N), (bits, kind, scans, chain_max, len(np.unique(want["score"])))
    t = table(db)
    got, st = t.linkage(kind)
    same(got, st, want, scans, chain_max, (bits, kind))
    again, _ = t.linkage(kind)
    assert again.tobytes() == got.tobytes(), "byte-identical from run to run"
    t.close()


def test_tversky():
    db, _ = scores_of(1024)
    S = score_matrix(db, TV)
    assert not np.isnan(S).any() and not np.array_equal(S, scores_of(1024)[1])
    t = table(db)
    for kind in KINDS:
        want = R.greedy(S, kind)
        _, scans, chain_max = R.chain(S, kind)
        assert not_vacuous(want, scans, chain_max, N)
        got, st = t.linkage(kind, **TV)
        same(got, st, want, scans, chain_max, ("tversky", kind))
    with pytest.raises(capi.GsimError) as e:
        t.linkage(0, metric=capi.METRIC_TVERSKY, alpha=0.3, beta=0.7)
    assert e.value.code == -1
    t.close()


@pytest.mark.parametrize("kind", KINDS)
def test_the_result_does_not_depend_on_launch_steps(kind):
    db, _ = scores_of(1024)
    want, scans, chain_max = expected(1024, kind)
    t = table(db)
    for steps in (1, 7, 0):
        got, st = t.linkage(kind, launch_steps=steps)
        same(got, st, want, scans, chain_max, (kind, steps))
        if steps:
            assert st["launch_steps"] == steps and st["launches"] == -(-scans // steps) > 100
        else:
            assert st["launch_steps"] > 7 and st["launches"] < scans // 7
    t.close()


def test_a_sub_range_with_a_row_base_and_the_search_state():
    lo, hi, base = 300, 2100, 7000
    db, S = scores_of(1024)
    sub = np.ascontiguousarray(S[lo:hi, lo:hi])
    t = table(db, base=base)
    singles = np.ascontiguousarray(db[[3, 500, N - 1]])

    def searches():
        hits, approx = t.search(singles, 50)
        return b"".join(h.tobytes() for h in hits) + approx.tobytes()

    before = searches()
    for kind in KINDS:
        want = R.greedy(sub, kind)
        _, scans, chain_max = R.chain(sub, kind)
        assert not_vacuous(want, scans, chain_max, hi - lo)
        got, st = t.linkage(kind, lo, hi)
        same(got, st, want, scans, chain_max, ("sub-range", kind), offset=lo + base)
        assert got["left"].max() == 2 * (hi - lo) - 3 and got["a"].min() >= lo + base and got["b"].max() < hi + base
        assert searches() == before, "the search state is as it was"
    for n in (0, 1):
        got, st = t.linkage(0, lo, lo + n)
        assert len(got) == 0 and st["rows"] == n and st["launches"] == 0
    with pytest.raises(capi.GsimError):
        t.linkage(0, 0, N + 1)  # a failed call ...
    assert searches() == before
    t.close()


def test_mst_cut_of_the_edges_is_the_cut_of_the_rule():
    db, _ = scores_of(1024)
    t = table(db)
    for kind in KINDS:
        want, _, _ = expected(1024, kind)
        got, _ = t.linkage(kind)
        edges = capi.linkage_edges(got)
        for level in (0.5, 1.0):
            component_of, first_row, sizes = capi.mst_cut(edges, N, level)
            rule = R.cut(want, N, level)
            assert 1 < len(first_row) < N and sizes.max() >= 1500
            assert np.array_equal(component_of, rule[0]) and np.array_equal(first_row, rule[1]) and np.array_equal(sizes, rule[2]), (kind, level)
    t.close()


def test_a_generated_table():
    """no host copy exists: the expected rows are regenerated with gsim_synth_row"""
    n, bits, seed = 1500, 1024, 0xC0131
    db = np.stack([capi.synth_row(seed, O.KIND_MORGAN, r, bits) for r in range(n)])
    S = score_matrix(db)
    S[np.isnan(S)] = 0
    generated = capi.Table(bits).generate(seed, O.KIND_MORGAN, 0, n, 0)
    for kind in KINDS:
        want = R.greedy(S, kind)
        _, scans, chain_max = R.chain(S, kind)
        assert len(np.unique(want["score"])) >= 100 and scans > n and chain_max >= 3
        got, st = generated.linkage(kind)
        same(got, st, want, scans, chain_max, ("generated", kind))
    generated.close()


def message():
    return capi.load().gsim_last_error().decode()


def refused(t, text):
    for kind in KINDS:
        with pytest.raises(capi.GsimError) as e:
            t.linkage(kind)
        assert e.value.code == -5 and message() == text, (e.value.code, message())


def small_rows():
    rng = np.random.default_rng(0x11A6)
    return np.packbits(rng.random((300, 1024)) < 0.25, axis=1, bitorder="little").view(np.uint32).copy()


def test_front_states():
    t = capi.Table(1024).add_rows(small_rows())
    with pytest.raises(capi.GsimError) as e:
        t.linkage(0)
    assert e.value.code == -5  # not finalized
    t.close()
    t = capi.Table(1024).add_rows(small_rows()).set_fold_factor(2).finalize(0, 1)
    refused(t, "linkage does not support folded tables")
    t.close()


def two_shards():
    t = capi.Table(1024).add_rows(small_rows()).finalize(0, 2)
    assert t.shard_count() == 2
    refused(t, "linkage needs a single-shard handle")
    t.close()


def test_two_shard_handles_are_refused():
    """Fewer than two GPUs: the same test in a child process on the test-hooks build with two logical devices on GPU 0."""
    if capi.device_count() >= 2:
        return two_shards()
    from conftest import hooks_env
    assert not os.environ.get("GSIM_TEST_ALIAS_DEVICES"), "two logical devices asked for, %d seen" % capi.device_count()
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "test_two_shard_handles_are_refused"], env=hooks_env(GSIM_TEST_ALIAS_DEVICES="2"),
                       capture_output=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0 and b"1 passed" in p.stdout, p.stdout.decode("utf-8", "replace")[-3000:]


# ---- past the 4 GiB offset: 24 distinct patterns x 1024 copies ----
GROUPS, COPIES = 24, 1024


def grouped_table():
    """(rows, the group of every row, the patterns' Tanimoto scores in the order of the groups' first rows)"""
    rng = np.random.default_rng(0x4617)
    patterns = np.packbits(rng.random((GROUPS, 1024)) < np.linspace(0.05, 0.4, GROUPS)[:, None], axis=1, bitorder="little").view(np.uint32).copy()
    group = np.repeat(np.arange(GROUPS), COPIES)[rng.permutation(GROUPS * COPIES)]
    firsts = np.array([np.flatnonzero(group == g)[0] for g in range(GROUPS)])
    order = np.argsort(firsts)  # groups by their lowest row
    rank = np.empty(GROUPS, np.int64)
    rank[order] = np.arange(GROUPS)
    group = rank[group]
    patterns = np.ascontiguousarray(patterns[order])
    P = np.stack([O.tanimoto_raw(patterns[g], patterns)[0] for g in range(GROUPS)]).astype(np.float32)
    assert not np.isnan(P).any() and len(np.unique(P[np.triu_indices(GROUPS, 1)])) > 200 and P[np.triu_indices(GROUPS, 1)].max() < 1
    return np.ascontiguousarray(patterns[group]), group, P


def grouped_expected(group, P, kind):
    """The first n - 24 merges, all at 1.0, in closed form from ORDER L -- the group of the lowest unmerged row is absorbed partner by
    partner in ascending row order, then the next group --, the last 23 from the rule on the 24 patterns with sizes 1024."""
    n = len(group)
    want = np.zeros(n - 1, R.MERGE_DTYPE)
    m = 0
    top = np.zeros(GROUPS, np.int64)  # the id of every group's cluster
    firsts = np.zeros(GROUPS, np.int64)
    for g in range(GROUPS):
        rows = np.flatnonzero(group == g)
        firsts[g] = rows[0]
        k = len(rows) - 1
        sl = slice(m, m + k)
        want["a"][sl] = rows[0]
        want["b"][sl] = rows[1:]
        want["left"][sl] = np.concatenate(([rows[0]], n + m + np.arange(k - 1)))
        want["right"][sl] = rows[1:]
        want["size"][sl] = 2 + np.arange(k)
        want["score"][sl] = 1.0
        want["sum_q"][sl] = (1 + np.arange(k)) * 2**31 if kind == capi.LINKAGE_AVERAGE else 2**31
        m += k
        top[g] = n + m - 1
    assert m == n - GROUPS and (np.diff(firsts) > 0).all()
    sizes = np.full(GROUPS, COPIES)
    tail = R.greedy(P, kind, sizes=sizes, sums=R.q(P) * COPIES * COPIES if kind == capi.LINKAGE_AVERAGE else None)
    ids = np.concatenate((top, n + m + np.arange(GROUPS - 1)))
    want[m:] = tail
    want["a"][m:] = firsts[tail["a"]]
    want["b"][m:] = firsts[tail["b"]]
    want["left"][m:] = ids[tail["left"]]
    want["right"][m:] = ids[tail["right"]]
    return want


@pytest.mark.parametrize("kind", [capi.LINKAGE_AVERAGE, capi.LINKAGE_COMPLETE])
def test_past_the_4_gib_offset(kind):
    """n = 24 576: the Q matrix of average linkage is 4.5 GiB; complete linkage (2.25 GiB) is the control below the offset"""
    db, group, P = grouped_table()
    n = len(db)
    assert n == 24576 and n * n * 8 > 2**32 > n * n * 4
    want = grouped_expected(group, P, kind)
    assert want["size"][-1] == n and (want["score"][:n - GROUPS] == 1.0).all() and len(np.unique(want["score"])) >= 20
    t = table(db)
    got, st = t.linkage(kind)
    assert got.tobytes() == want.tobytes(), (kind, np.flatnonzero(got != want)[:5], got[:3], want[:3])
    assert st["scans"] > 2 * n and st["merges"] == n - 1
    t.close()
