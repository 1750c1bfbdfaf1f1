"""CPU checks of the threshold-join entry points (gsim_db_join_queries, gsim_db_join, gsim_graph_get_join_stats): every
argument error the header lists is reported BEFORE any device state -- so it holds on a machine with no GPU -- and a table
whose rows are not on a GPU is a state error, never a host computation."""
import ctypes as C

import numpy as np
import pytest

from gpusimilarity_amd import capi

TV = capi.METRIC_TVERSKY


def small(bits=1024, n=4):
    W = bits // 32
    return capi.Table(bits).add_rows(np.arange(n * W, dtype=np.uint32).reshape(n, W))


def invalid(fn, *a, **kw):
    with pytest.raises(capi.GsimError) as e:
        fn(*a, **kw)
    assert e.value.code == -1, (a, kw, e.value)
    assert len(str(e.value)) > len("gsim error -1: "), "an error without a message"


def test_symbols_and_constants():
    L = capi.load()
    for name in ("gsim_db_join_queries", "gsim_db_join", "gsim_graph_get_join_stats"):
        assert hasattr(L, name) and name in capi.EXPORTS
    assert (capi.JOIN_BY_ROW, capi.JOIN_BY_SCORE) == (0, 1)
    assert C.sizeof(capi.GsimJoinStats) == 12 * 8


@pytest.mark.parametrize("left_is_handle", [False, True])
def test_argument_errors_come_before_the_device(left_is_handle):
    t = small()
    left = small() if left_is_handle else np.ones((3, 32), np.uint32)
    for bad in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        invalid(t.join, left, bad)
    invalid(t.join, left, 0.5, metric=7)
    invalid(t.join, left, 0.5, order=2)
    invalid(t.join, left, 0.5, order=-1)
    for al, be in ((-0.1, 0.5), (0.5, -0.1), (float("nan"), 0.5), (0.5, float("inf")), (float("-inf"), 1.0)):
        invalid(t.join, left, 0.5, metric=TV, alpha=al, beta=be)
    # (Tanimoto ignores alpha / beta, as gsim_db_search does)
    with pytest.raises(capi.GsimError) as e:
        t.join(left, 0.5, alpha=-1.0, beta=float("nan"))
    assert e.value.code == -5
    wide = small(4096 + 32, 2)
    invalid(wide.join, small(4096 + 32, 2) if left_is_handle else np.zeros((1, 129), np.uint32), 0.5)


def test_handle_ranges_widths_and_null_arguments():
    t, left = small(), small(n=6)
    invalid(t.join, left, 0.5, row_begin=3, row_end=2)
    invalid(t.join, left, 0.5, row_begin=0, row_end=7)
    invalid(t.join, left, 0.5, row_begin=7, row_end=7)
    invalid(t.join, small(512), 0.5)  # different fp_bits
    L = capi.load()
    g = C.c_void_p(123)
    q = np.ones(32, np.uint32)
    assert L.gsim_db_join_queries(None, capi._u32(q), 1, 0.5, 0, 1.0, 1.0, 0, C.byref(g)) == -1
    assert L.gsim_db_join_queries(t._h, capi._u32(q), 1, 0.5, 0, 1.0, 1.0, 0, None) == -1
    assert L.gsim_db_join_queries(t._h, None, 1, 0.5, 0, 1.0, 1.0, 0, C.byref(g)) == -1
    assert g.value is None  # *out is cleared on failure
    assert L.gsim_db_join_queries(t._h, capi._u32(q), 1 << 32, 0.5, 0, 1.0, 1.0, 0, C.byref(g)) == -1
    assert b"2^32" in L.gsim_last_error()
    assert L.gsim_db_join(None, left._h, 0, 1, 0.5, 0, 1.0, 1.0, 0, C.byref(g)) == -1
    assert L.gsim_db_join(t._h, None, 0, 1, 0.5, 0, 1.0, 1.0, 0, C.byref(g)) == -1
    assert L.gsim_db_join(t._h, left._h, 0, 1, 0.5, 0, 1.0, 1.0, 0, None) == -1
    assert L.gsim_db_join(t._h, left._h, 1 << 40, (1 << 40) + (1 << 33), 0.5, 0, 1.0, 1.0, 0, C.byref(g)) == -1
    assert L.gsim_graph_get_join_stats(None, None) == -1
    st = capi.GsimJoinStats()
    assert L.gsim_graph_get_join_stats(None, C.byref(st)) == -1


def test_rows_not_on_a_gpu_are_a_state_error():
    t, left = small(), small()
    cases = [dict(), dict(metric=TV, alpha=0.5, beta=0.5), dict(metric=TV, alpha=1.0, beta=0.0), dict(metric=TV, alpha=0.3, beta=0.7),
             dict(order=capi.JOIN_BY_SCORE), dict(row_begin=1, row_end=3)]
    for kw in cases:
        for lf in (left, t, np.ones((2, 32), np.uint32), np.ones(32, np.uint32)):
            with pytest.raises(capi.GsimError) as e:
                t.join(lf, 0.5, **kw)
            assert e.value.code == -5, kw
    # ... even for a call without left rows (the state is checked before the empty result is made)
    with pytest.raises(capi.GsimError) as e:
        t.join(np.zeros((0, 32), np.uint32), 0.5)
    assert e.value.code == -5


def test_python_twin_has_join_and_screen():
    from gpusimilarity_amd.fingerprintdb import FingerprintDB
    assert callable(FingerprintDB.join) and callable(FingerprintDB.screen)
