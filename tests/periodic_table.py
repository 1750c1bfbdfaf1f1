"""A host model of a PERIODIC table, the reference of tests/test_gpu_large_offsets.py: a table far too large for a CPU oracle to scan
(17 GiB, 216 M rows) whose every result can still be worked out in O(period).

Row r of the table is block[r % P] with P = 4099, a prime -- unless r is one of a few PLANTED rows, which hold given fingerprints.
P is prime, so a displacement by a power of two (a byte offset or a word index that wrapped at 2^31 or 2^32, a row number cut to 24
bits) lands on another block row: a wrap cannot read identical data.

The table therefore has only U = P + len(planted) distinct SOURCES: source u < P is block row u (held by every row r = u mod P that
is not planted), source P + i is the i-th planted row (ascending by row number).  The oracle (oracle_lib, a *_rule.py) runs on the
U source rows (`sources()`), and one helper per result shape turns that per-source result into the whole table's:

    expand_vector   a per-row value (a label, a score, a weighted popcount)         np.take(per_source, source_of(rows))
    expand_counts   column counts over the whole table                              sum(multiplicity(u) * bits(source u))
    expand_hist     a histogram row                                                 sum(multiplicity(u) * onehot(bin of source u))
    expand_csr      hit lists (threshold lists by row; top-k lists by score, row)   a source's hit -> all its replicas, in row order
    expand_label_counts   per-label column counts for labels r % period with planted overrides

`wrapped(boundary, shift)` is the NEGATIVE CONTROL: the same table as a kernel with a wrapped offset would see it -- every row at or
past `boundary` reads row r - shift.  tests/test_periodic_model_host.py checks every helper against the real oracles on a
materialised table, and that each shape's result over the wrapped table differs from the true one.

Nothing here calls the library under test."""
import numpy as np

import oracle_lib as O

P = 4099
F32 = np.float32


def dense_family(seed, W, nvariants):
    """A random dense fingerprint F and its variants: variant j is F with its j lowest set bits cleared (variant 0 is F), so that the
    scores against F descend strictly: popc(F) - j common bits of popc(F).  -> uint32 [nvariants, W]."""
    F = O.synth_rows(seed, O.KIND_DENSE, 0, 1, W)[0]
    bits = np.unpackbits(F.view(np.uint8), bitorder="little")
    on = np.flatnonzero(bits)
    assert len(on) > nvariants
    out = np.empty((nvariants, W), np.uint32)
    for j in range(nvariants):
        b = bits.copy()
        b[on[:j]] = 0
        out[j] = np.packbits(b, bitorder="little").view(np.uint32)
    return out


def plant(n, W, boundaries, seed, tail=20):
    """The planting scheme -> (planted {row: fingerprint}, info dict).  `boundaries`: ascending row numbers, each the first row past
    some offset.
    (a) the dense family, 2 * len(boundaries) + tail variants: two at rows b - 1 and b of every boundary b (a run that straddles it)
        and `tail` in the last rows of the table; variant j sits in family slot (11 j) mod nslots (slots ascending by row), which
        scatters the best variants over the boundary runs and the tail;
    (b) an all-ones row at b + 1 of every boundary;
    (c) an all-zero row just below the tail."""
    boundaries = [int(b) for b in boundaries]
    assert boundaries == sorted(boundaries) and boundaries[0] >= 2 and boundaries[-1] + 2 < n - tail - 1
    slots = [r for b in boundaries for r in (b - 1, b)] + list(range(n - tail, n))
    ns = len(slots)
    assert ns >= 20 and np.gcd(11, ns) == 1
    fam = dense_family(seed ^ 0xFA111, W, ns)
    planted, variant_row = {}, np.empty(ns, np.int64)
    for j in range(ns):
        r = slots[(11 * j) % ns]
        planted[r] = fam[j]
        variant_row[j] = r
    ones = [b + 1 for b in boundaries]
    for r in ones:
        planted[r] = np.full(W, 0xFFFFFFFF, np.uint32)
    zero = n - tail - 1
    planted[zero] = np.zeros(W, np.uint32)
    assert len(planted) == ns + len(ones) + 1
    return planted, dict(family=fam, variant_row=variant_row, ones=ones, zero=zero, boundaries=boundaries, tail=(n - tail, n))


class PeriodicTable:
    def __init__(self, n, W, seed, planted, wrap=None):
        self.n, self.W, self.seed = int(n), int(W), seed
        self.block = O.synth_rows(seed, O.KIND_SPARSE, 0, P, W)
        self.prow = np.array(sorted(planted), np.int64)
        assert len(self.prow) == 0 or (self.prow[0] >= 0 and self.prow[-1] < n)
        self.pfp = (np.stack([np.asarray(planted[int(r)], np.uint32) for r in self.prow]) if len(self.prow)
                    else np.zeros((0, W), np.uint32))
        self.U = P + len(self.prow)
        self.wrap = wrap  # (boundary row, shift) of the negative control
        self._planted = planted
        self._by_source = None

    def wrapped(self, boundary, shift):
        assert 0 < shift <= boundary < self.n
        return PeriodicTable(self.n, self.W, self.seed, self._planted, wrap=(int(boundary), int(shift)))

    # ---- the rows
    def sources(self):
        """uint32 [U, W]: the distinct rows -- what the oracle scans instead of the table"""
        return np.concatenate([self.block, self.pfp])

    def source_of(self, rows):
        """the source index of each table row"""
        r = np.asarray(rows, np.int64)
        if self.wrap is not None:
            r = np.where(r >= self.wrap[0], r - self.wrap[1], r)
        src = r % P
        if len(self.prow):
            i = np.searchsorted(self.prow, r)
            hit = self.prow[np.minimum(i, len(self.prow) - 1)] == r
            src = np.where(hit, P + i, src)
        return src

    def row(self, r):
        return self.rows(r, r + 1)[0]

    def rows(self, lo, hi):
        """uint32 [hi - lo, W]: the rows of [lo, hi) materialised"""
        assert 0 <= lo <= hi <= self.n
        return self.sources()[self.source_of(np.arange(lo, hi))]

    def take_rows(self, rows):
        return self.sources()[self.source_of(rows)]

    # ---- how often, and where, a source occurs
    def _generic(self):
        if self._by_source is None:
            assert self.n <= 1 << 24, "the generic path materialises the source of every row"
            src = self.source_of(np.arange(self.n))
            order = np.argsort(src, kind="stable")
            starts = np.searchsorted(src[order], np.arange(self.U + 1))
            self._by_source = (order, starts)
        return self._by_source

    def multiplicity(self, u, generic=False):
        """how many rows hold source u: for a block row the rows r < n with r % P == u, minus the planted ones; 1 for a planted row"""
        if generic or self.wrap is not None:
            _, starts = self._generic()
            return int(starts[u + 1] - starts[u])
        if u >= P:
            return 1
        return (self.n - u + P - 1) // P - int((self.prow % P == u).sum())

    def multiplicities(self, generic=False):
        """int64 [U]"""
        if generic or self.wrap is not None:
            _, starts = self._generic()
            return np.diff(starts).astype(np.int64)
        m = (self.n - np.arange(P) + P - 1) // P
        np.subtract.at(m, self.prow % P, 1)
        return np.concatenate([m, np.ones(len(self.prow), np.int64)])

    def replicas(self, u, limit=None, generic=False):
        """the ascending row numbers that hold source u (the first `limit` of them)"""
        if generic or self.wrap is not None:
            order, starts = self._generic()
            return order[starts[u]:starts[u + 1]][:limit].astype(np.int64)
        if u >= P:
            return self.prow[u - P:u - P + 1][:limit]
        mine = self.prow[self.prow % P == u]
        stop = self.n if limit is None else min(self.n, u + P * (limit + len(mine)))
        r = np.arange(u, stop, P, dtype=np.int64)
        return r[~np.isin(r, mine)][:limit]

    # ---- the expansions
    def expand_vector(self, per_source, lo=0, hi=None):
        """per_source [U] -> the value of every row of [lo, hi)"""
        hi = self.n if hi is None else hi
        per_source = np.asarray(per_source)
        assert per_source.shape[0] == self.U
        if self.wrap is None and hi - lo > 1 << 22:  # whole large tables: tile the period, then the planted rows
            out = np.tile(per_source[:P], (hi - lo + P - 1) // P + 1)[lo % P:lo % P + hi - lo]
            mine = (self.prow >= lo) & (self.prow < hi)
            out[self.prow[mine] - lo] = per_source[P:][mine]
            return out
        return np.take(per_source, self.source_of(np.arange(lo, hi)), axis=0)

    def expand_counts(self):
        """-> (counts uint64 [W * 32], counted): how many rows of the table have each bit set"""
        return (self.multiplicities().astype(np.uint64) @ unpack(self.sources()).astype(np.uint64)), self.n

    def expand_hist(self, bins, nbins, self_rows=None):
        """bins int [nl, U]: the bin of (left row i, source u) -> hist uint64 [nl, nbins] over the whole table.  self_rows[i]: left row i
        IS that table row and the pair is not counted (exclude_self)."""
        m = self.multiplicities()
        hist = np.zeros((len(bins), nbins), np.int64)
        for i, b in enumerate(bins):
            np.add.at(hist[i], b, m)
        if self_rows is not None:
            own = self.source_of(self_rows)
            hist[np.arange(len(bins)), bins[np.arange(len(bins)), own]] -= 1
        assert hist.min() >= 0 and (hist.sum(axis=1) == self.n - (self_rows is not None)).all()
        return hist.astype(np.uint64)

    def expand_csr(self, S, cutoff, k=None, self_rows=None):
        """S f32 [nl, U]: score(left row i, source u) -> CSR (indptr uint64, indices uint32, scores f32).  List i holds the table rows
        whose source scores >= cutoff (a NaN never does): every replica of such a source.  k = None: a threshold list, by row.
        k: a k-NN list, by (score descending, row ascending), cut to k -- a boundary tie group keeps its lowest rows.
        self_rows[i]: left row i IS that table row, which is left out of its own list."""
        S = np.asarray(S, F32)
        assert S.shape[1] == self.U
        cut = F32(cutoff)
        indptr, ind, sc = [0], [], []
        for i in range(len(S)):
            with np.errstate(invalid="ignore"):
                srcs = np.flatnonzero(S[i] >= cut)
            limit = None if k is None else k + (self_rows is not None)
            reps = [self.replicas(u, limit) for u in srcs]
            rows = np.concatenate(reps) if reps else np.zeros(0, np.int64)
            s = np.repeat(S[i, srcs], [len(r) for r in reps]).astype(F32)
            if self_rows is not None:
                keep = rows != int(self_rows[i])
                rows, s = rows[keep], s[keep]
            order = np.argsort(rows, kind="stable") if k is None else np.lexsort((rows, -s.astype(np.float64)))[:k]
            ind.append(rows[order].astype(np.uint32))
            sc.append(s[order])
            indptr.append(indptr[-1] + len(order))
        return (np.array(indptr, np.uint64), np.concatenate(ind) if ind else np.zeros(0, np.uint32),
                np.concatenate(sc) if sc else np.zeros(0, F32))

    def expand_label_counts(self, period, nlabels, planted_labels):
        """Labels: row r has label r % period, except the planted rows, which have planted_labels[i] (ascending by row; LABEL_NONE =
        0xFFFFFFFF: counted nowhere) -> (counts uint32 [nlabels, W * 32], sizes uint32 [nlabels]).  P is prime to `period`, so the
        pair (r % P, r % period) has the period P * period and every combination occurs."""
        assert self.wrap is None and np.gcd(P, period) == 1 and period <= nlabels and len(planted_labels) == len(self.prow)
        x = np.arange(P * period)
        cnt = (self.n - x + P * period - 1) // (P * period)  # the rows r < n with r % (P * period) == x
        pairs = np.zeros((period, P), np.int64)              # pairs[l, u]: rows of label l that are copies of block row u
        np.add.at(pairs, (x % period, x % P), cnt)
        np.subtract.at(pairs, (self.prow % period, self.prow % P), 1)
        assert pairs.min() >= 0
        counts = np.zeros((nlabels, self.W * 32), np.int64)
        counts[:period] = pairs @ unpack(self.block).astype(np.int64)
        sizes = np.zeros(nlabels, np.int64)
        sizes[:period] = pairs.sum(axis=1)
        pb = unpack(self.pfp).astype(np.int64)
        for i, l in enumerate(planted_labels):
            if int(l) != 0xFFFFFFFF:
                counts[int(l)] += pb[i]
                sizes[int(l)] += 1
        return counts.astype(np.uint32), sizes.astype(np.uint32)

    def labels(self, period, planted_labels, lo=0, hi=None):
        """the label vector that expand_label_counts counts, for the rows of [lo, hi)"""
        hi = self.n if hi is None else hi
        lab = (np.arange(lo, hi, dtype=np.int64) % period).astype(np.uint32)
        mine = (self.prow >= lo) & (self.prow < hi)
        lab[self.prow[mine] - lo] = np.asarray(planted_labels, np.uint32)[mine]
        return lab


def unpack(rows):
    """rows x fp_bits 0/1 bytes: bit k is bit k % 32 of word k // 32"""
    rows = np.ascontiguousarray(rows, dtype="<u4")
    return np.unpackbits(rows.view(np.uint8).reshape(len(rows), -1), axis=1, bitorder="little")


def cutoff_between(S_block, S_family):
    """The cutoff that the family tests use: asserted on the CPU that NO block row reaches it against any left row and that EVERY
    planted variant does.  It is the f32 half-way between the best block score and the worst variant score."""
    best_block, worst_variant = float(np.max(S_block)), float(np.min(S_family))
    cutoff = float(F32((best_block + worst_variant) / 2))
    assert best_block < cutoff <= worst_variant, (best_block, cutoff, worst_variant)
    assert not (np.asarray(S_block, F32) >= F32(cutoff)).any() and (np.asarray(S_family, F32) >= F32(cutoff)).all()
    return cutoff


# ---- the inputs that the host tests of the model and the GPU tests share
TAN = dict()
TV = dict(metric=O.METRIC_TVERSKY, alpha=0.5, beta=0.5)
METRICS = [TAN, TV]
TINY = float(np.nextafter(F32(0), F32(1)))  # the smallest positive float: "every row with a non-zero score"


def score_matrix(left, model, kw=TAN):
    """S[i, u] = the oracle's f32 score of left row i (the query) against source u"""
    import kmeans_rule
    return kmeans_rule.score_matrix(np.ascontiguousarray(left, dtype=np.uint32), model.sources(), kw)


def family_sources(model, info):
    """the source index of every variant of the family, by variant"""
    return P + np.searchsorted(model.prow, info["variant_row"])


def family_cutoff(S, model, info):
    """cutoff_between for a score matrix over the sources: block rows against the family's variants"""
    return cutoff_between(S[:, :P], S[:, family_sources(model, info)])


def family_left(info):
    """F and two of its variants"""
    return np.ascontiguousarray(info["family"][[0, 3, 7]])


def mixed_left(model, info):
    """70 left rows of every sort: 40 copies of block rows, 20 variants of the family, 8 fresh rows (dense and sparse), all ones, all zero"""
    W = model.W
    left = np.concatenate([model.block[(np.arange(40) * 97 + 5) % P], info["family"][:20],
                           O.synth_rows(model.seed ^ 0x0DD, O.KIND_DENSE, 0, 4, W), O.synth_rows(model.seed ^ 0x0DD, O.KIND_SPARSE, 7, 4, W),
                           np.full((1, W), 0xFFFFFFFF, np.uint32), np.zeros((1, W), np.uint32)])
    assert len(left) == 70
    return np.ascontiguousarray(left)


def centres(model, info):
    """130 centres -- two centre blocks of the assignment kernel: 129 block rows and F (the last)"""
    return np.ascontiguousarray(np.concatenate([model.block[(np.arange(129) * 31 + 1) % P], info["family"][:1]]))


def straddles(model, info, half):
    """row ranges of 2 * half rows around every boundary, and the last 2 * half rows"""
    return [(b - half, b + half) for b in info["boundaries"]] + [(model.n - 2 * half, model.n)]


def boundary_rowset(model, info, half):
    """a row set: the planted rows and `half` rows on either side of every boundary, and the table's last rows; ascending"""
    parts = [np.arange(lo, hi) for lo, hi in straddles(model, info, half)] + [model.prow]
    return np.unique(np.concatenate(parts))


def data_edges(S):
    """histogram edges that bite: five distinct scores that occur below 1, then 1.0"""
    u = np.unique(S[(S > 0) & (S < 1)])
    assert len(u) >= 5
    e = np.array([u[int(q * (len(u) - 1))] for q in (0.1, 0.3, 0.5, 0.7, 0.9)] + [1.0], F32)
    assert (np.diff(e) > 0).all()
    return e


def hist_bins(S, edges):
    """the bin of a score: the number of edges e with s >= e"""
    return np.searchsorted(np.asarray(edges, F32), S, side="right")


def mean_in_order(S):
    """the MEAN group score: an f32 sum in query order, one rounding per step, then one division"""
    acc = np.zeros(S.shape[1], F32)
    for i in range(S.shape[0]):
        acc = (acc + S[i]).astype(F32)
    return (acc / F32(S.shape[0])).astype(F32)


def past(rows, info):
    """non-vacuity of an expected result: at least 20 of its rows lie at or past the last boundary, and one at or past each"""
    rows = np.asarray(rows, np.int64)
    b = info["boundaries"]
    assert int((rows >= b[-1]).sum()) >= 20, "fewer than 20 expected rows past the last boundary"
    for lo, hi in zip(b, b[1:] + [1 << 62]):
        assert ((rows >= lo) & (rows < hi)).any(), "no expected row between boundaries %d and %d" % (lo, hi)
