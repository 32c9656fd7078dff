"""Host side of predict_similar_items_top_k (tensorrec_amd/similar.py): id validation, k_fetch and the batch plan -- no GPU."""
import numpy as np
import pytest

from tensorrec_amd import similar as S


def test_none_expands_to_every_item_in_order():
    ids64, ids32, all_items = S.query_ids(None, 7)
    assert all_items
    assert ids64.dtype == np.int64 and ids32.dtype == np.int32
    assert np.array_equal(ids64, np.arange(7)) and np.array_equal(ids32, np.arange(7))


@pytest.mark.parametrize("ids", [[6, 12, 6, 0, 12], np.array([6, 12, 6, 0, 12], np.int16), np.array([6, 12, 6, 0, 12], np.uint64),
                                 (6, 12, 6, 0, 12)])
def test_repeats_and_order_are_kept(ids):
    ids64, ids32, all_items = S.query_ids(ids, 13)
    assert not all_items
    assert ids64.dtype == np.int64 and ids32.dtype == np.int32
    assert ids64.tolist() == [6, 12, 6, 0, 12] and ids32.tolist() == [6, 12, 6, 0, 12]


def test_id_of_n_items_is_refused():
    with pytest.raises(ValueError):
        S.query_ids([0, 5], 5)
    assert S.query_ids([0, 4], 5)[0].tolist() == [0, 4]


def test_negative_id_is_refused():
    with pytest.raises(ValueError):
        S.query_ids([3, -1], 5)


def test_non_integer_ids_and_shapes_are_refused():
    with pytest.raises(ValueError):
        S.query_ids([0.0, 1.0], 5)
    with pytest.raises(ValueError):
        S.query_ids(np.array([True, False]), 5)
    with pytest.raises(ValueError):
        S.query_ids(np.zeros((2, 2), np.int64), 5)


def test_empty_list_gives_empty_ids():
    ids64, ids32, all_items = S.query_ids([], 5)
    assert not all_items and ids64.shape == (0,) and ids32.shape == (0,)
    assert ids64.dtype == np.int64 and ids32.dtype == np.int32


def test_k_below_one_is_refused():
    for k in (0, -3):
        with pytest.raises(ValueError):
            S.check_k(k)
    assert S.check_k(np.int64(4)) == 4 and isinstance(S.check_k(np.int64(4)), int)


def test_k_fetch():
    assert S.k_fetch(10, False) == 10
    assert S.k_fetch(10, True) == 11
    assert S.k_fetch(16, True) == 17                       # (not clamped at a route's largest k: the route is chosen for 17)
    assert S.k_fetch(64, True) == 65
    assert S.k_fetch(64, True, slab_route=True) == 64      # (the slab route masks its slabs: nothing fetched on top)
    assert S.k_fetch(64, False, slab_route=True) == 64


def test_batch_plan():
    assert S.batch_plan(20000, 7000) == [(0, 7000), (7000, 14000), (14000, 20000)]
    assert S.batch_plan(5, 5) == [(0, 5)] and S.batch_plan(5, 9) == [(0, 5)]
    assert S.batch_plan(5, None) == [(0, 5)]
    assert S.batch_plan(0, None) == [] and S.batch_plan(0, 3) == []
    with pytest.raises(ValueError):
        S.batch_plan(5, 0)
