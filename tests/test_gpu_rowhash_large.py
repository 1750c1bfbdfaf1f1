"""gsim_rowhash_* on a table past the 2^32-byte offset: 35.7 M rows of 1024 bits (4.3 GiB), built as tests/test_gpu_large_offsets.py
builds its tables -- the 4099-row block of tests/periodic_table.py repeated, planted rows around the rows whose byte offsets are 2^31
and 2^32.  Every row is a replica of row r mod P or a planted row, so first, size and the stats follow from the model in O(P), and a
lookup of the P block rows must answer with rows below P.  The negative control: the model's wrapped(boundary, shift) table -- what
a kernel whose byte offset wrapped at 2^32 would read -- gives another `first` for every row past the boundary, so such a kernel
cannot pass.  The groups hold 8 700 rows each: thousands of rows race for each of 4099 slots."""
import numpy as np
import pytest

import periodic_table as T
import rowhash_rule as R
from gpusimilarity_amd import capi

pytestmark = pytest.mark.gpu
P = T.P
GIB = 1 << 30
SEED = 0x9E1
W = 32
N = (1 << 25) + (1 << 21) + 3
BOUNDARIES = [1 << 23, 1 << 24, 1 << 25, (1 << 25) + (1 << 20)]
NEED = 9 * GIB  # the table, the index (1 GiB of slots, 0.3 GiB of groups) and room to spare


class Large:
    def __init__(self):
        import torch
        free = capi.device_free_bytes(0)
        if free < NEED:
            pytest.skip("needs %.0f GiB of free HBM, %.0f GiB free" % (NEED / GIB, free / GIB))
        assert [BOUNDARIES[1] * W * 4, BOUNDARIES[2] * W * 4] == [1 << 31, 1 << 32]
        planted, self.info = T.plant(N, W, BOUNDARIES, SEED)
        self.model = m = T.PeriodicTable(N, W, SEED, planted)
        block = torch.from_numpy(m.block.view(np.int32)).cuda()
        self.ten = block.repeat((N + P - 1) // P, 1)[:N]
        self.ten.index_copy_(0, torch.from_numpy(m.prow).cuda(), torch.from_numpy(m.pfp.view(np.int32)).cuda())
        torch.cuda.synchronize()
        assert tuple(self.ten.shape) == (N, W) and self.ten.is_contiguous()
        self.table = capi.Table(W * 32).attach_device_rows(self.ten.data_ptr(), N, 0)
        self.ix = self.table.rowhash()
        # the model's groups: the classes of identical sources, their lowest rows and their sizes
        src = m.sources()
        _, cls = np.unique(src, axis=0, return_inverse=True)
        cls = cls.reshape(-1)
        lowest = np.array([m.replicas(u, 1)[0] for u in range(m.U)], np.int64)
        mult = m.multiplicities()
        cfirst = np.full(cls.max() + 1, N, np.int64)
        np.minimum.at(cfirst, cls, lowest)
        csize = np.zeros(cls.max() + 1, np.int64)
        np.add.at(csize, cls, mult)
        self.cls, self.first_of_source, self.size_of_source = cls, cfirst[cls].astype(np.uint32), csize[cls].astype(np.uint32)
        self.ngroups, self.nrepeated = int(cls.max() + 1), int((csize >= 2).sum())

    def close(self):
        import torch
        self.ix.close()
        self.table.close()
        del self.ten
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def large():
    x = Large()
    yield x
    x.close()


def test_groups_and_stats_are_the_models(large):
    m = large.model
    first, size = large.ix.groups()
    want_first, want_size = m.expand_vector(large.first_of_source), m.expand_vector(large.size_of_source)
    assert first.tobytes() == want_first.tobytes(), np.flatnonzero(first != want_first)[:5]
    assert size.tobytes() == want_size.tobytes(), np.flatnonzero(size != want_size)[:5]
    st = large.ix.stats()
    assert st["rows"] == N and st["groups"] == large.ngroups and st["slots"] == 1 << 27 == R.slots(N)
    assert m.U - 8 < large.ngroups <= m.U, "the sources are distinct but for the all-ones rows"
    assert st["repeated_groups"] == large.nrepeated >= P and st["largest_group"] == int(large.size_of_source.max()) and 8000 < st["largest_group"] < 9000
    assert (want_first[BOUNDARIES[2]:] < P).sum() > (1 << 21) - 100, "rows past the 2^32-byte offset belong to groups that begin in the first block"
    print("rowhash large: build kernel_ms %.2f wall_ms %.1f" % (st["kernel_ms"], st["wall_ms"]))
    rs = large.ix.rowset()
    assert rs.count == large.ngroups and np.array_equal(rs.rows(), np.flatnonzero(want_first == np.arange(N, dtype=np.uint32)))
    rs.close()


def test_a_wrapped_offset_would_show(large):
    """the negative control: were the rows at or past the 2^32-byte offset read 2^32 bytes lower, every one of them would get another
    first row -- and the index's answer is the true one"""
    m = large.model
    boundary = shift = BOUNDARIES[2]
    assert boundary * W * 4 == 1 << 32 and shift % P != 0
    bad = m.wrapped(boundary, shift)
    rows = np.arange(boundary, N)
    true = large.first_of_source[m.source_of(rows)]
    wrapped = large.first_of_source[bad.source_of(rows)]
    assert (true != wrapped).mean() > 0.999 and len(rows) > 1 << 21
    first, _ = large.ix.groups()
    assert np.array_equal(first[boundary:], true)


def test_find_answers_with_rows_of_the_first_block_and_the_planted_rows(large):
    m = large.model
    q = np.concatenate([m.block, m.pfp, m.block[:40] ^ np.uint32(1 << 7)])
    row, size = large.ix.find(q)
    assert np.array_equal(row[:P], large.first_of_source[:P]) and (row[:P] < P).all()
    assert np.array_equal(size[:P], large.size_of_source[:P])
    assert np.array_equal(row[P:m.U], large.first_of_source[P:]) and np.array_equal(size[P:m.U], large.size_of_source[P:])
    assert (row[P:m.U] >= BOUNDARIES[2]).sum() >= 20, "rows found past the 2^32-byte offset"
    absent = R.find(m.sources(), q[m.U:])[0] == R.ROW_NONE
    assert absent.sum() >= 30 and (row[m.U:][absent] == R.ROW_NONE).all() and (size[m.U:][absent] == 0).all()
    # the table's own rows on either side of every boundary
    for b in BOUNDARIES:
        r, s = large.ix.find_db(large.table, b - 3, b + 3)
        src = m.source_of(np.arange(b - 3, b + 3))
        assert np.array_equal(r, large.first_of_source[src]) and np.array_equal(s, large.size_of_source[src])
