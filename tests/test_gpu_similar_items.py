"""predict_similar_items_top_k (docs/similar_items.md): the k most similar items of every query item, ranked on the device by the
exact top-k routes of predict_top_k.  The reference for row q is row q of ``recommendation_graphs.predict_similar_items`` -- the
matrix the old method brings to the host -- with column ids[q] set to -inf when the query itself is excluded, selected by the
oracle's top-k (value descending, ties by ascending id); values and ids must be bit-identical.  The models are biased (random
item biases), so a bias that leaked into the item-item scores would show in every comparison."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

import tensorrec_amd as T  # noqa: E402
from tensorrec_amd import ops  # noqa: E402
from tensorrec_amd import recommendation_graphs as R  # noqa: E402
from tensorrec_amd.prediction_graphs import (AbstractPredictionGraph, DotProductPredictionGraph,  # noqa: E402
                                             CosineSimilarityPredictionGraph, EuclideanSimilarityPredictionGraph)
from tensorrec_amd.representation_graphs import LinearRepresentationGraph  # noqa: E402


def _model(n_items, d, graph, precision="fp32", n_users=8, n_item_features=None):
    """tests/test_gpu_routes.py::_model: seeded weights, random biases; with identity features item_repr is the weight table"""
    m = T.TensorRec(n_components=d, prediction_graph=graph(), user_repr_graph=LinearRepresentationGraph(),
                    item_repr_graph=LinearRepresentationGraph(), seed=0, precision=precision)
    m.build(n_users, n_items if n_item_features is None else n_item_features)
    w = m.get_weights()
    rng = np.random.default_rng(1)
    for name in ("user_feature_biases", "item_feature_biases"):
        w[name] = (0.05 * rng.standard_normal(w[name].shape)).astype(np.float32)
    m.set_weights(w)
    return m


def _eye(n):
    return sp.identity(n, dtype=np.float32, format="csr")


def _reference(model, itf, ids, k, exclude_self):
    """(values [len(ids), kk], ids [len(ids), kk]) of the definition, kk = min(k, items left in a row)"""
    ids = np.asarray(ids, np.int64)
    item_repr = torch.from_numpy(model.predict_item_representation(itf)).cuda()
    dense = R.predict_similar_items(model.prediction_graph_factory, item_repr, ids).cpu().numpy()
    if exclude_self:
        dense[np.arange(len(ids)), ids] = -np.inf
    kk = min(k, dense.shape[1] - (1 if exclude_self else 0))
    return O.topk_rows(dense, kk)


def _check_rows(model, itf, ids, rows, vals, idx, k, exclude_self):
    rv, ri = _reference(model, itf, np.asarray(ids)[rows], k, exclude_self)
    kk = rv.shape[1]
    assert np.array_equal(idx[rows][:, :kk], ri) and np.array_equal(vals[rows][:, :kk], rv)
    assert np.all(idx[rows][:, kk:] == -1) and np.all(np.isneginf(vals[rows][:, kk:]))


@pytest.mark.parametrize("graph", [DotProductPredictionGraph, CosineSimilarityPredictionGraph, EuclideanSimilarityPredictionGraph])
@pytest.mark.parametrize("exclude_self", [False, True])
def test_direct_route_every_row(graph, exclude_self):
    n, k = 1682, 10
    m, itf = _model(n, 64, graph), _eye(n)
    vals, idx, rep = m.predict_similar_items_top_k(itf, k=k, exclude_self=exclude_self, return_route=True)
    assert rep["route"] == "direct" and rep == m.last_route and rep["k"] == k
    assert rep["similar"] == {"n_queries": n, "exclude_self": exclude_self, "k_fetch": k + 1 if exclude_self else k}
    assert vals.shape == (n, k) and idx.shape == (n, k) and vals.dtype == np.float32 and idx.dtype == np.int32
    _check_rows(m, itf, np.arange(n), np.arange(n), vals, idx, k, exclude_self)
    if graph is CosineSimilarityPredictionGraph:
        if exclude_self:
            assert not np.any(idx == np.arange(n)[:, None])
        else:
            assert np.array_equal(idx[:, 0], np.arange(n))


def test_ties_and_self_among_duplicates():
    """Items 100..139 share one feature row: 40 identical representations, all tied at the top of each other's rows.  Only the
    query's own column leaves; 139's own id is not among its 11 fetched places (100..110), so nothing is dropped there."""
    n, k = 3000, 10
    cols = np.arange(n)
    cols[100:140] = 100
    itf = sp.csr_matrix((np.ones(n, np.float32), (np.arange(n), cols)), shape=(n, n))
    m = _model(n, 64, CosineSimilarityPredictionGraph)
    ids = [100, 139, 105]
    vals, idx = m.predict_similar_items_top_k(itf, ids, k=k, exclude_self=True)
    assert idx[0].tolist() == list(range(101, 111))
    assert idx[1].tolist() == list(range(100, 110))
    assert idx[2].tolist() == [100, 101, 102, 103, 104, 106, 107, 108, 109, 110]
    _check_rows(m, itf, ids, np.arange(3), vals, idx, k, True)
    vals, idx = m.predict_similar_items_top_k(itf, ids, k=k)
    assert all(row.tolist() == list(range(100, 110)) for row in idx)
    _check_rows(m, itf, ids, np.arange(3), vals, idx, k, False)


def _pinned(m, itf, ids, k, route, exclude_self=False, k_fetch=None):
    vals, idx, rep = m.predict_similar_items_top_k(itf, ids, k=k, exclude_self=exclude_self, return_route=True)
    n_q = itf.shape[0] if ids is None else len(ids)
    assert rep["route"] == route and rep == m.last_route, rep
    assert rep["similar"]["k_fetch"] == (k if k_fetch is None else k_fetch) and rep["similar"]["n_queries"] == n_q
    assert vals.shape == (n_q, k) and idx.shape == (n_q, k)
    return vals, idx


def test_routes_cascade_and_wide_cascade_by_k_fetch():
    n = 300_000
    m, itf = _model(n, 128, DotProductPredictionGraph), _eye(n)
    ids = np.random.default_rng(5).integers(0, n, 512)
    ids[1], ids[-1] = ids[0], ids[3]                          # repeats
    rows = np.r_[0:8, 504:512]
    vals, idx = _pinned(m, itf, ids, 10, "cascade_int8")
    _check_rows(m, itf, ids, rows, vals, idx, 10, False)
    # 16 places without the query = 17 fetched: the wide cascade's k, not the narrow cascade clamped at its 16
    vals, idx = _pinned(m, itf, ids, 16, "wide_cascade", exclude_self=True, k_fetch=17)
    _check_rows(m, itf, ids, rows, vals, idx, 16, True)


def test_route_bf16_filter():
    n = 100_000
    m, itf = _model(n, 64, DotProductPredictionGraph), _eye(n)
    ids = np.random.default_rng(6).integers(0, n, 300)
    for ex in (False, True):
        vals, idx = _pinned(m, itf, ids, 10, "bf16_filter", exclude_self=ex, k_fetch=11 if ex else 10)
        _check_rows(m, itf, ids, np.r_[0:8, 292:300], vals, idx, 10, ex)


def test_route_euclid_certified():
    n = 20_000
    m, itf = _model(n, 64, EuclideanSimilarityPredictionGraph), _eye(n)
    ids = np.random.default_rng(7).integers(0, n, 300)
    for ex in (False, True):
        vals, idx = _pinned(m, itf, ids, 10, "euclid_certified", exclude_self=ex, k_fetch=11 if ex else 10)
        _check_rows(m, itf, ids, np.r_[0:8, 292:300], vals, idx, 10, ex)


def test_route_slab_and_places_beyond_the_catalogue():
    n = 3000
    m, itf = _model(n, 64, DotProductPredictionGraph), _eye(n)
    ids = [5, 2999, 5, 0]
    for ex in (False, True):                                  # (the slab route masks the query's column: nothing fetched on top)
        vals, idx = _pinned(m, itf, ids, 100, "slab", exclude_self=ex, k_fetch=100)
        _check_rows(m, itf, ids, np.arange(4), vals, idx, 100, ex)
    n = 50
    m, itf = _model(n, 16, CosineSimilarityPredictionGraph), _eye(n)
    vals, idx = _pinned(m, itf, None, 64, "slab", exclude_self=True, k_fetch=64)
    assert np.all(idx[:, 49:] == -1) and np.all(np.isneginf(vals[:, 49:])) and np.all(idx[:, :49] >= 0)
    _check_rows(m, itf, np.arange(n), np.arange(n), vals, idx, 64, True)
    # ... and on a fused route: 12 places + the query fetched from 10 items, 9 of them left
    n = 10
    m, itf = _model(n, 16, CosineSimilarityPredictionGraph), _eye(n)
    vals, idx = _pinned(m, itf, None, 12, "direct", exclude_self=True, k_fetch=13)
    _check_rows(m, itf, np.arange(n), np.arange(n), vals, idx, 12, True)


def test_bf16_precision_takes_the_bf16_route():
    n = 20_000
    m, itf = _model(n, 64, DotProductPredictionGraph, precision="bf16"), _eye(n)
    _pinned(m, itf, np.arange(0, n, 97), 10, "two_stage")     # (approximate scores: shapes and route only, as the routes test does)


def test_batches_and_device_results():
    n, k = 20_000, 10
    m, itf = _model(n, 64, CosineSimilarityPredictionGraph), _eye(n)
    for ex in (False, True):
        v1, i1, r1 = m.predict_similar_items_top_k(itf, k=k, exclude_self=ex, return_route=True)
        v3, i3, r3 = m.predict_similar_items_top_k(itf, k=k, exclude_self=ex, item_batch_size=7000, return_route=True)
        assert r1["user_batch_size"] >= n and r3["user_batch_size"] == 7000
        assert np.array_equal(v1, v3) and np.array_equal(i1, i3)
        vd, idd = m.predict_similar_items_top_k(itf, k=k, exclude_self=ex, item_batch_size=7000, return_device=True)
        assert vd.is_cuda and idd.is_cuda and vd.dtype == torch.float32 and idd.dtype == torch.int32
        assert np.array_equal(vd.cpu().numpy(), v1) and np.array_equal(idd.cpu().numpy(), i1)
    _check_rows(m, itf, np.arange(n), np.r_[0:8, 6996:7004, n - 8:n], v1, i1, k, True)


def test_agrees_with_predict_similar_items_on_untied_data():
    n = 1682
    m, itf = _model(n, 64, CosineSimilarityPredictionGraph), _eye(n)
    old = m.predict_similar_items(itf, [6, 12], 5)
    vals, idx = m.predict_similar_items_top_k(itf, [6, 12], k=5)
    assert [[int(i) for i, _ in row] for row in old] == idx.tolist()
    assert np.array_equal(np.array([[s for _, s in row] for row in old], np.float32), vals)


def test_arguments():
    n = 150
    m, itf = _model(n, 16, DotProductPredictionGraph), _eye(n)
    for bad in ([0, n], [-1], np.array([3, n + 5])):
        with pytest.raises(ValueError):
            m.predict_similar_items_top_k(itf, bad)
    with pytest.raises(ValueError):
        m.predict_similar_items_top_k(itf, [1], k=0)
    with pytest.raises(ValueError):
        m.predict_similar_items_top_k(itf, [1], item_batch_size=0)
    vals, idx, rep = m.predict_similar_items_top_k(itf, [], k=7, return_route=True)
    assert vals.shape == (0, 7) and idx.shape == (0, 7) and vals.dtype == np.float32 and idx.dtype == np.int32
    assert rep["similar"]["n_queries"] == 0

    class Custom(AbstractPredictionGraph):
        def connect_dense_prediction_graph(self, tf_user_representation, tf_item_representation):
            return tf_user_representation @ tf_item_representation.t()

        def connect_serial_prediction_graph(self, tf_user_representation, tf_item_representation, tf_x_user, tf_x_item):
            return (tf_user_representation[tf_x_user.long()] * tf_item_representation[tf_x_item.long()]).sum(dim=1)

    mc = _model(n, 16, Custom)
    with pytest.raises(ValueError):
        mc.predict_similar_items_top_k(itf, [1])


def _drop_self_numpy(vals, idx, self_ids):
    k = idx.shape[1] - 1
    ov, oi = np.empty((len(idx), k), np.float32), np.empty((len(idx), k), np.int32)
    for r in range(len(idx)):
        hit = np.nonzero(idx[r] == self_ids[r])[0]
        keep = np.delete(np.arange(k + 1), hit[0] if len(hit) else k)
        ov[r], oi[r] = vals[r, keep], idx[r, keep]
    return ov, oi


@pytest.mark.parametrize("kf", [2, 11, 17, 65, ops.EXCLUDE_K_MAX + 1])
def test_topk_drop_self_kernel(kf):
    """Row r places its own id by r % 5: first place, last place, a middle place, absent, inside a padded row."""
    n = 1000
    rng = np.random.default_rng(kf)
    idx = np.argsort(rng.random((n, 2 * kf + 8)), axis=1)[:, :kf].astype(np.int32)          # distinct ids per row
    vals = -np.sort(-rng.standard_normal((n, kf)).astype(np.float32), axis=1)
    vals[::7, : kf // 2 + 1] = 0.5                                                          # (tied scores change nothing)
    self_ids = np.empty(n, np.int32)
    for r in range(n):
        case = r % 5
        if case == 4:
            n_real = max(1, kf // 2)
            vals[r, n_real:], idx[r, n_real:] = -np.inf, -1
            self_ids[r] = idx[r, n_real // 2]
        else:
            self_ids[r] = (idx[r, 0], idx[r, kf - 1], idx[r, kf // 2], 1_000_000)[case]
    ov, oi = ops.topk_drop_self(torch.from_numpy(vals).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(self_ids).cuda())
    rv, ri = _drop_self_numpy(vals, idx, self_ids)
    assert ov.shape == (n, kf - 1) and oi.shape == (n, kf - 1)
    assert np.array_equal(oi.cpu().numpy(), ri) and np.array_equal(ov.cpu().numpy(), rv)
