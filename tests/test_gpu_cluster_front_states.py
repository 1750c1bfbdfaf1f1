"""The state errors of the clustering fronts that came after the single-table list (tests/test_gpu_single_front_states.py has the
first fifteen): a folded table and a handle of two shards are refused by every entry point that can get that far, with
GSIM_ERR_STATE, exactly the text the entry point had before its checks were shared (literal strings below, copied from that source;
check_table_state's `plural` differs per call: "core scores do not ...", "hdbscan does not ..."), and the outputs cleared that the
front clears before it looks at the state.

gsim_db_search_labels cannot reach either message: it needs a label set of the handle, and gsim_labelset_create refuses such a handle.

Two shards: on two GPUs or, on one, in a child process on the test-hooks build with two logical devices on GPU 0."""
import os
import subprocess
import sys

import pytest

import cluster_front_errors_cases as cases
from gpusimilarity_amd import capi
from test_gpu_single_front_states import BITS, INVALID, N, ROOT, STATE, message, rows

pytestmark = pytest.mark.gpu

FOLDED = {
    "dbscan": "dbscan does not support folded tables",
    "core_scores": "core scores do not support folded tables",
    "mreach_mst": "mreach mst does not support folded tables",
    "hdbscan": "hdbscan does not support folded tables",
    "label_sums": "label sums do not support folded tables",
    "labelset_create": "label sets do not support folded tables",
    "linkage": "linkage does not support folded tables",
    "snn": "snn does not support folded tables",
    "jarvis_patrick": "jarvis-patrick does not support folded tables",
}
SHARDED = {
    "dbscan": "dbscan needs a single-shard handle",
    "core_scores": "core scores need a single-shard handle",
    "mreach_mst": "mreach mst needs a single-shard handle",
    "hdbscan": "hdbscan needs a single-shard handle",
    "label_sums": "label sums need a single-shard handle",
    "labelset_create": "label sets need a single-shard handle",
    "linkage": "linkage needs a single-shard handle",
    "snn": "snn needs a single-shard handle",
    "jarvis_patrick": "jarvis-patrick needs a single-shard handle",
}
# what a front has cleared by the time it looks at the state (the others are left as they were; label sums write their stats only
# behind the state check)
CLEARED = {
    "dbscan": {"nclusters": "zero", "stats": "zero"}, "core_scores": {"stats": "zero"}, "mreach_mst": {"nedges": "zero", "stats": "zero"},
    "hdbscan": {"nclusters": "zero", "stats": "zero"}, "label_sums": {}, "labelset_create": {"out": "cleared"},
    "linkage": {"nmerges": "zero", "stats": "zero"}, "snn": {"out": "cleared"}, "jarvis_patrick": {"stats": "zero"},
}


def refused(table, texts):
    """Every entry point of `texts` refuses `table` with its text; then the table is closed."""
    c = cases.Calls(bits=BITS, rows=N, table=table)
    assert set(texts) == set(CLEARED) and len(texts) == 9
    for entry, text in texts.items():
        code, out = getattr(c, entry)()
        assert code == STATE and message() == text, (entry, code, message())
        for name, state in out.items():
            if (entry, name) == ("jarvis_patrick", "nclusters"):  # the three levels of the call, of the eight the buffer has room for
                assert state[:3] == [0, 0, 0] and state[3] == 0xA5A5A5A5, state
                continue
            want = CLEARED[entry].get(name, "untouched")
            assert state == want, (entry, name, state)
    # the label search: no label set of this handle can be made, and another handle's is an argument error
    code, _ = c.search_labels(ls="other")
    assert code == INVALID and message() == "the label set was made for another handle"
    c.close()


def test_folded_tables_are_refused_with_each_entry_points_text():
    t = capi.Table(BITS).add_rows(rows()).set_fold_factor(2).finalize(0, 1)
    assert t.fold_factor() == 2 and t.shard_count() == 1
    refused(t, FOLDED)


def test_a_folded_handle_of_two_shards_is_called_folded():
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
