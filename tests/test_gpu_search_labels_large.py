"""gsim_db_search_labels on the smallest table past the 2^32-byte offset: 8 400 000 rows of 4096 bits, 4.3 GB.

The table is tests/test_gpu_large_offsets.py's kind: the 4099-row block of tests/periodic_table.py repeated, planted rows written over
it (a dense family straddling the 2^31- and 2^32-byte boundaries and in the table's last rows, all-ones rows, an all-zero row), built
by torch and handed over with gsim_db_attach_device_rows -- its content owes nothing to the code under test.  Labels: row r has label
r % 4099 -- so a label's unplanted rows are the copies of ONE block row, its best is the lowest of them, and a row read from a wrapped
offset (another block row: 4099 is prime) shows as a foreign score in the label -- with planted overrides: every second variant goes
to a label of the family's own, the others keep r % 4099, one all-ones row is GSIM_LABEL_NONE, the others share a label, the all-zero
row joins label 5.

Expected values in O(period): the oracle scores the 4099 + 29 distinct SOURCES; a label's candidates are its block row (first copy,
number of copies) and the planted rows given to it.  The negative control, on the model alone: the table as a kernel with an offset
wrapped at 2^32 bytes would see it gives other bests and other counts."""
import numpy as np
import pytest

import periodic_table as T
import search_labels_rule as R
from gpusimilarity_amd import capi

pytestmark = pytest.mark.gpu
P = T.P
N, W = 8_400_000, 128
BOUNDARIES = [1 << 22, 1 << 23]  # the first rows at byte offsets 2^31 and 2^32
SEED = 0x5EA
NONE = capi.LABEL_NONE
FAMILY_LABEL, ONES_LABEL, NLABELS = P, P + 1, P + 2
K = 60


class Model:
    def __init__(self):
        assert [b * W * 4 for b in BOUNDARIES] == [1 << 31, 1 << 32] and N * W * 4 > (1 << 32) + (5 << 20)
        planted, self.info = T.plant(N, W, BOUNDARIES, SEED)
        self.m = m = T.PeriodicTable(N, W, SEED, planted)
        variant_of = {int(r): j for j, r in enumerate(self.info["variant_row"])}
        lab = []
        for r in m.prow:
            r = int(r)
            if r in variant_of:
                lab.append(FAMILY_LABEL if variant_of[r] % 2 == 0 else r % P)
            elif r in self.info["ones"]:
                lab.append(NONE if r == self.info["ones"][0] else ONES_LABEL)
            else:
                assert r == self.info["zero"]
                lab.append(5)
        self.planted_labels = np.array(lab, np.uint32)
        self.queries = np.ascontiguousarray(np.concatenate([self.info["family"][[0, 3]], m.block[[5, 1000]], np.full((1, W), 0xFFFFFFFF, np.uint32),
                                                            np.zeros((1, W), np.uint32)]))
        src = m.sources()
        self.S = np.nan_to_num(T.score_matrix(self.queries, m), nan=0.0).astype(np.float32)
        # the selective cutoff, from the expected values: the median score of a block row against the block -- about half of the labels
        # keep rows for the two block-row queries, all of them for the dense family's
        self.cutoff = float(np.median(self.S[2, :P]))
        bits = T.unpack(src)
        self.popc = bits.sum(axis=1).astype(np.uint16)
        self.common = (T.unpack(self.queries).astype(np.uint16) @ bits.T.astype(np.uint16)).astype(np.uint16)
        # a label's candidates: (label, source, first row, rows) -- the block row of every label, then the planted rows that have one
        first = np.array([m.replicas(u, 1)[0] for u in range(P)], np.int64)
        given = self.planted_labels != NONE
        self.e_label = np.concatenate([np.arange(P), self.planted_labels[given]]).astype(np.int64)
        self.e_source = np.concatenate([np.arange(P), P + np.flatnonzero(given)])
        self.e_row = np.concatenate([first, m.prow[given]])
        self.e_rows = np.concatenate([m.multiplicities()[:P], np.ones(int(given.sum()), np.int64)])
        assert self.e_rows.sum() == N - 1 and (first == np.arange(P)).all()

    def labels(self):
        return self.m.labels(P, self.planted_labels)

    def expect(self, k, cutoff):
        nq = len(self.queries)
        out = dict(hits=np.zeros((nq, k), dtype=R.HIT), hit_labels=np.zeros((nq, k), np.uint32), counts=np.zeros(nq, np.uint32),
                   approx=np.zeros(nq, np.uint64), rows_kept=np.zeros(nq, np.uint64), label_best=np.full((nq, NLABELS), R.NO_HIT, dtype=R.HIT),
                   label_kept=np.zeros((nq, NLABELS), np.uint32))
        for q in range(nq):
            s = R.after_cutoff(self.S[q, self.e_source], cutoff)
            keep = np.ones(len(s), bool) if cutoff <= 0 else s != 0
            idx = np.flatnonzero(keep)
            out["label_kept"][q] = np.bincount(self.e_label[idx], weights=self.e_rows[idx], minlength=NLABELS).astype(np.uint32)
            order = idx[np.lexsort((self.e_row[idx], -s[idx].astype(np.float64)))]
            labs, pos = np.unique(self.e_label[order], return_index=True)
            best = order[pos]
            rec = np.zeros(len(best), dtype=R.HIT)
            rec["row"], rec["score"] = self.e_row[best], s[best]
            rec["common"], rec["popc_db"] = self.common[q, self.e_source[best]], self.popc[self.e_source[best]]
            out["label_best"][q, labs] = rec
            top = self.e_label[order[np.sort(pos)]][:k]
            out["hits"][q, :len(top)] = out["label_best"][q, top]
            out["hit_labels"][q, :len(top)] = top
            out["counts"][q], out["approx"][q], out["rows_kept"][q] = len(top), len(labs), out["label_kept"][q].sum()
        return out

    def best_block_scores(self, q, cutoff, wrap=None):
        """per label r % P: (the greatest score, the number of kept rows) over the unplanted rows, of the table as it is or as a kernel
        that wraps would see it (every row materialised: 8.4 M scores, one query)"""
        m = self.m.wrapped(*wrap) if wrap else self.m
        s = R.after_cutoff(self.S[q, m.source_of(np.arange(N))], cutoff)
        s[self.m.prow] = 0.0
        pad = np.zeros(-N % P, np.float32)
        s = np.concatenate([s, pad]).reshape(-1, P)
        return s.max(axis=0), (s != 0).sum(axis=0)


@pytest.fixture(scope="module")
def model():
    return Model()


@pytest.fixture(scope="module")
def big(model):
    import torch
    m = model.m
    block = torch.from_numpy(m.block.view(np.int32)).cuda()
    ten = block.repeat((N + P - 1) // P, 1)[:N]
    ten.index_copy_(0, torch.from_numpy(m.prow).cuda(), torch.from_numpy(m.pfp.view(np.int32)).cuda())
    torch.cuda.synchronize()
    assert ten.dtype == torch.int32 and tuple(ten.shape) == (N, W) and ten.is_contiguous() and ten.numel() * 4 > 1 << 32
    t = capi.Table(W * 32).attach_device_rows(ten.data_ptr(), N, 0)
    ls = t.labelset(model.labels(), NLABELS)
    yield t, ls
    ls.close()
    t.close()
    del ten
    torch.cuda.empty_cache()


def test_the_wrapped_table_gives_another_result(model):
    """the negative control, on the model alone"""
    wrap = (BOUNDARIES[1], BOUNDARIES[1])
    for q in (2, 3):
        true_best, true_kept = model.best_block_scores(q, model.cutoff)
        assert np.array_equal(true_best, R.after_cutoff(model.S[q, :P], model.cutoff)), "a label's unplanted rows are the copies of one block row"
        assert P / 4 <= (true_best != 0).sum() <= 3 * P / 4, "between a quarter and three quarters of the labels keep a row"
        wrong_best, wrong_kept = model.best_block_scores(q, model.cutoff, wrap)
        assert (wrong_best != true_best).sum() >= 20 and (wrong_kept != true_kept).sum() >= 20, "an offset wrapped at 2^32 bytes shows"
    w = model.expect(K, 0.0)
    for q in (0, 1):
        rows = w["label_best"][q]["row"].astype(np.int64)
        rows = rows[rows != 0xFFFFFFFF]
        assert (rows >= BOUNDARIES[1]).sum() >= 8 and ((rows >= BOUNDARIES[0]) & (rows < BOUNDARIES[1])).any(), "bests on either side of the boundaries"
        assert (w["hits"][q]["row"][:10] >= BOUNDARIES[0] - 1).all(), "the family's variants lead the list"
    assert w["label_best"][0, FAMILY_LABEL]["score"] == 1.0 and w["label_kept"][0, FAMILY_LABEL] == 12
    assert w["label_kept"][0, ONES_LABEL] == 1 and w["rows_kept"][0] == N - 1, "one all-ones row is labelled nowhere"


@pytest.mark.parametrize("selective", [False, True])
def test_the_large_table_matches_the_model(big, model, selective):
    t, ls = big
    cutoff = model.cutoff if selective else 0.0
    sizes, labelled, nonempty = ls.sizes()
    assert labelled == N - 1 and nonempty == NLABELS
    w = model.expect(K, cutoff)
    got = t.search_labels(ls, model.queries, K, cutoff, per_label=True, stats=True)
    R.same(got, w, cutoff)
    assert got["stats"]["passes_lds"] >= 1 and got["stats"]["passes_global"] == 0 and got["stats"]["launches"] >= 3
    if cutoff <= 0:
        assert np.array_equal(got["label_kept"][0], sizes)
    cut = t.search_labels(ls, model.queries, K, cutoff, per_label=True, launch_rows=1 << 21)  # five launches: the boundaries inside two of them
    R.same(cut, w, (cutoff, "cut"))
