"""The state errors of the single-table fronts that need a table on a GPU (capi_front.h check_table_state): a folded table and a
handle of two shards are refused by every entry point that can get that far, with GSIM_ERR_STATE, exactly the text the entry point
had before the check was shared (literal strings below, copied from that source), and the outputs cleared that the front clears
before it looks at the state.  A handle that is both folded and sharded is called folded by all of them -- gsim_db_knn used to say
"single-shard" there.

gsim_db_search_rows cannot reach either message: it needs a row set of the handle, and the constructors refuse such a handle.

Two shards: on two GPUs or, on one, in a child process on the test-hooks build with two logical devices on GPU 0."""
import os
import subprocess
import sys

import numpy as np
import pytest

import single_front_errors_cases as cases
from gpusimilarity_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE, INVALID = -5, -1
N, BITS = 300, 1024

FOLDED = {
    "neighbors": "neighbour lists do not support folded tables",
    "knn": "knn does not support folded tables",
    "maxmin": "maxmin does not support folded tables",
    "leader": "leader clustering does not support folded tables",
    "components": "components do not support folded tables",
    "mst": "mst does not support folded tables",
    "bit_counts": "column counts do not support folded tables",
    "overlap_sums": "column counts do not support folded tables",
    "assign": "assign does not support folded tables",
    "label_counts": "label counts does not support folded tables",
    "kmeans": "k-means does not support folded tables",
    "search_group": "group searches do not support folded tables",
    "rowset_from_rows": "row sets do not support folded tables",
    "rowset_from_bitmap": "row sets do not support folded tables",
}
SHARDED = {
    "neighbors": "neighbour lists need a single-shard handle",
    "knn": "knn needs a single-shard handle",
    "maxmin": "maxmin needs a single-shard handle",
    "leader": "leader clustering needs a single-shard handle",
    "components": "components need a single-shard handle",
    "mst": "mst needs a single-shard handle",
    "bit_counts": "column counts need a single-shard handle",
    "overlap_sums": "column counts need a single-shard handle",
    "assign": "assign needs a single-shard handle",
    "label_counts": "label counts needs a single-shard handle",
    "kmeans": "k-means needs a single-shard handle",
    "search_group": "group searches need a single-shard handle",
    "rowset_from_rows": "row sets need a single-shard handle",
    "rowset_from_bitmap": "row sets need a single-shard handle",
}
# what a front has cleared by the time it looks at the state (the others are left as they were; assign, label_counts and k-means
# write their stats only behind the state check)
CLEARED = {
    "neighbors": {"out": "cleared"}, "knn": {"out": "cleared"}, "rowset_from_rows": {"out": "cleared"}, "rowset_from_bitmap": {"out": "cleared"},
    "maxmin": {"npicked": "zero", "stats": "zero"}, "leader": {"nleaders": "zero", "stats": "zero"}, "components": {"stats": "zero"},
    "mst": {"nedges": "zero", "stats": "zero"}, "bit_counts": {"counted": "zero", "stats": "zero"}, "overlap_sums": {"stats": "zero"},
    "assign": {}, "label_counts": {}, "kmeans": {}, "search_group": {"stats": "zero"},
}


def rows():
    rng = np.random.default_rng(0x51F7)
    return np.packbits(rng.random((N, BITS)) < 0.25, axis=1, bitorder="little").view(np.uint32).copy()


def message():
    return capi.load().gsim_last_error().decode()


def refused(table, texts):
    """Every entry point of `texts` refuses `table` with its text; then the table is closed."""
    c = cases.Calls(bits=BITS, rows=N, table=table)
    assert set(texts) == set(CLEARED) and len(texts) == 14
    for entry, text in texts.items():
        code, out = getattr(c, entry)()
        assert code == STATE and message() == text, (entry, code, message())
        for name, state in out.items():
            if (entry, name) == ("components", "ncomponents"):  # the three levels of the call, of the eight the buffer has room for
                assert state[:3] == [0, 0, 0] and state[3] == 0xA5A5A5A5, state
                continue
            want = CLEARED[entry].get(name, "untouched")
            assert state == want, (entry, name, state)
    # the row-set search: no row set of this handle can be made, and another handle's is an argument error
    code, _ = c.search_rows(rs="other")
    assert code == INVALID and message() == "the row set was made for another handle"
    c.close()


def test_folded_tables_are_refused_with_each_entry_points_text():
    t = capi.Table(BITS).add_rows(rows()).set_fold_factor(2).finalize(0, 1)
    assert t.fold_factor() == 2 and t.shard_count() == 1
    refused(t, FOLDED)


def test_a_folded_handle_of_two_shards_is_called_folded():
    """One order for all, fold first.  (A folded table has one shard per add_rows slice, on whichever devices.)"""
    db = rows()
    t = capi.Table(BITS).add_rows(db[:150]).add_rows(db[150:]).set_fold_factor(2).finalize(0, 1)
    assert t.shard_count() == 2 and t.fold_factor() == 2 and t.count() == N
    refused(t, FOLDED)


def two_shards():
    t = capi.Table(BITS).add_rows(rows()).finalize(0, 2)
    assert t.shard_count() == 2 and t.fold_factor() == 1
    refused(t, SHARDED)


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
