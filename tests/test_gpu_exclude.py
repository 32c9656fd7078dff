"""predict_top_k(exclude=...) and predict_rank_of_interactions(exclude=...) on the GPU (docs/exclusion.md): every route against
the top-k of the dense prediction with the excluded ids dropped in NumPy (model.predict is bit-exact vs the oracle elsewhere),
the route pinned through return_route; the masked selection kernel on hand-made rows; filtered pair ranks against the oracle's
ranks minus the excluded items ahead."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

import tensorrec_amd as T  # noqa: E402
from tensorrec_amd import ops  # noqa: E402
from tensorrec_amd.prediction_graphs import DotProductPredictionGraph, EuclideanSimilarityPredictionGraph  # noqa: E402
from tensorrec_amd.representation_graphs import LinearRepresentationGraph  # noqa: E402


def _model(n_users, n_items, d, graph=DotProductPredictionGraph, precision="fp32", tie_pairs=(), **kw):
    m = T.TensorRec(n_components=d, prediction_graph=graph(), user_repr_graph=LinearRepresentationGraph(),
                    item_repr_graph=LinearRepresentationGraph(), seed=0, precision=precision, **kw)
    m.build(n_users, n_items)
    w = m.get_weights()
    rng = np.random.default_rng(1)
    for name in ("user_feature_biases", "item_feature_biases"):
        w[name] = (0.05 * rng.standard_normal(w[name].shape)).astype(np.float32)
    for a, b in tie_pairs:                    # identical items: equal scores for every user (ties across the exclusion)
        for name in w:
            if name.endswith("item") or name == "item_feature_biases":
                w[name][b] = w[name][a]
    m.set_weights(w)
    return m


def _eye(n):
    return sp.identity(n, dtype=np.float32, format="csr")


def _excl_matrix(n_users, n_items, per_user):
    """csr [n_users, n_items] with ones at per_user[u] (a list of id arrays)."""
    rows = np.concatenate([np.full(len(p), u) for u, p in enumerate(per_user)]).astype(np.int64)
    cols = np.concatenate([np.asarray(p, np.int64) for p in per_user])
    m = sp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n_users, n_items))
    m.sum_duplicates()
    return m


def _expected(pred, excl_rows, k):
    """First k places of (value desc, index asc) of each row of pred after dropping excl_rows[u]; -inf / -1 beyond."""
    n, ni = pred.shape
    ev = np.full((n, k), -np.inf, np.float32)
    ei = np.full((n, k), -1, np.int32)
    for u in range(n):
        keep = np.ones(ni, bool)
        keep[np.asarray(excl_rows[u], np.int64)] = False
        cols = np.nonzero(keep)[0]
        v = pred[u, cols]
        o = np.lexsort((cols, -v))[:k]
        ev[u, :len(o)], ei[u, :len(o)] = v[o], cols[o]
    return ev, ei


def _rows_of(m, users):
    m = sp.csr_matrix(m)
    return [m.indices[m.indptr[u]:m.indptr[u + 1]][m.data[m.indptr[u]:m.indptr[u + 1]] != 0] for u in users]


def _check(model, uf, itf, k, route, excl, users=None):
    vals, idx, rep = model.predict_top_k(uf, itf, k=k, exclude=excl, return_route=True)
    assert rep["route"] == route and rep == model.last_route, rep
    assert vals.shape == (uf.shape[0], k) and idx.shape == (uf.shape[0], k)
    users = np.arange(uf.shape[0]) if users is None else np.asarray(users)
    pred = model.predict(uf[users], itf)
    ev, ei = _expected(pred, _rows_of(excl, users), k)
    assert np.array_equal(idx[users], ei) and np.array_equal(vals[users], ev)
    return rep


def _true_top(model, uf, itf, k):
    return model.predict_top_k(uf, itf, k=k)[1]


def test_direct_route_configs1_shape():
    """943 x 1,682, d = 64 (configs[1]): users without exclusions, users with all but 3 items excluded (padding, tier 2), and
    excluded items that tie with non-excluded ones (identical item rows)."""
    nu, ni = 943, 1682
    ties = [(5, 6), (7, 8), (100, 101)]
    m = _model(nu, ni, 64, tie_pairs=ties)
    rng = np.random.default_rng(2)
    top = _true_top(m, _eye(nu), _eye(ni), 16)
    per = []
    for u in range(nu):
        if u < 100:
            per.append([])
        elif u < 130:
            per.append(np.setdiff1d(np.arange(ni), rng.choice(ni, 3, replace=False)))
        else:
            a, b = ties[u % 3]
            per.append(np.unique(np.concatenate([rng.choice(ni, 20, replace=False), [a if u % 2 else b], top[u, [0, 2]]])))
    excl = _excl_matrix(nu, ni, per)
    rep = _check(m, _eye(nu), _eye(ni), 10, "direct", excl)
    assert rep["exclude"]["k_fetch"] == 16 and rep["exclude"]["n_excluded"] == excl.nnz
    assert rep["exclude"]["n_fallback"] >= 30                   # (at least the users with 3 items left)


def test_heavy_exclusion_every_user_falls_back():
    """Each user's own top-50 excluded: no user keeps 10 of its 16 fetched places, every user is re-done on a masked slab."""
    nu, ni = 943, 1682
    m = _model(nu, ni, 64)
    pred = m.predict(_eye(nu), _eye(ni))
    top50 = O.topk_rows(pred, 50)[1]
    excl = _excl_matrix(nu, ni, list(top50))
    rep = _check(m, _eye(nu), _eye(ni), 10, "direct", excl)
    assert rep["exclude"]["n_fallback"] == nu


@pytest.fixture(scope="module")
def big():
    nu, ni = 512, 1_000_000
    return _model(nu, ni, 128), _eye(nu), _eye(ni)


def test_cascade_int8_1m_items(big):
    """configs[2]'s route (int8 -> bf16 -> fp32 cascade), k = 10: each user's true 3rd and 7th best and 30 random items excluded"""
    m, uf, itf = big
    nu, ni = uf.shape[0], itf.shape[0]
    top = _true_top(m, uf, itf, 10)
    rng = np.random.default_rng(3)
    excl = _excl_matrix(nu, ni, [np.concatenate([top[u, [2, 6]], rng.choice(ni, 30, replace=False)]) for u in range(nu)])
    rep = _check(m, uf, itf, 10, "cascade_int8", excl, users=[0, 1, 200, 511])
    assert rep["exclude"]["k_fetch"] == 16


def test_wide_cascade_k32_1m_items(big):
    m, uf, itf = big
    nu, ni = uf.shape[0], itf.shape[0]
    top = _true_top(m, uf, itf, 32)
    rng = np.random.default_rng(4)
    excl = _excl_matrix(nu, ni, [np.concatenate([top[u, [0, 5, 31]], rng.choice(ni, 17, replace=False)]) for u in range(nu)])
    rep = _check(m, uf, itf, 32, "wide_cascade", excl, users=[3, 300])
    assert 32 < rep["exclude"]["k_fetch"] <= 64


def test_euclid_certified_with_item_biases():
    nu, ni = 300, 30_000
    m = _model(nu, ni, 64, EuclideanSimilarityPredictionGraph)
    top = _true_top(m, _eye(nu), _eye(ni), 10)
    rng = np.random.default_rng(5)
    per = [np.concatenate([top[u, :2], rng.choice(ni, 5 if u % 4 else 40, replace=False)]) for u in range(nu)]
    rep = _check(m, _eye(nu), _eye(ni), 10, "euclid_certified", _excl_matrix(nu, ni, per), users=np.arange(0, nu, 10))
    assert rep["exclude"]["k_fetch"] == 12


def test_multi_taste_merge():
    nu, ni = 300, 1682
    m = _model(nu, ni, 32, n_tastes=3)
    top = _true_top(m, _eye(nu), _eye(ni), 10)
    rng = np.random.default_rng(6)
    per = [np.concatenate([top[u, :3] if u % 3 else top[u], rng.choice(ni, 4, replace=False)]) for u in range(nu)]
    rep = _check(m, _eye(nu), _eye(ni), 10, "direct", _excl_matrix(nu, ni, per))
    assert rep["exclude"]["n_fallback"] > 0


def test_attention_slab_route_k100():
    nu, ni = 64, 3000
    m = _model(nu, ni, 16, n_tastes=2, attention_graph=LinearRepresentationGraph())
    top = _true_top(m, _eye(nu), _eye(ni), 20)
    rng = np.random.default_rng(7)
    per = [np.concatenate([top[u], rng.choice(ni, 50, replace=False)]) if u % 8 else np.arange(ni - 40) for u in range(nu)]
    rep = _check(m, _eye(nu), _eye(ni), 100, "slab", _excl_matrix(nu, ni, per))
    assert rep["exclude"]["k_fetch"] == 100 and rep["exclude"]["n_fallback"] == 0


def test_bf16_two_stage():
    """bf16 precision: exact on the bf16 score matrix the route scores with (model.predict of a bf16 model)"""
    nu, ni = 256, 20_000
    m = _model(nu, ni, 64, precision="bf16")
    top = _true_top(m, _eye(nu), _eye(ni), 16)
    rng = np.random.default_rng(8)
    per = [np.concatenate([top[u, :3] if u % 2 else top[u], rng.choice(ni, 10, replace=False)]) for u in range(nu)]
    rep = _check(m, _eye(nu), _eye(ni), 10, "two_stage", _excl_matrix(nu, ni, per), users=np.arange(0, nu, 16))
    assert rep["exclude"]["n_fallback"] > 0


def test_none_and_all_zero_exclude_change_nothing():
    nu, ni = 200, 1682
    m = _model(nu, ni, 64)
    uf, itf = _eye(nu), _eye(ni)
    v0, i0, r0 = m.predict_top_k(uf, itf, k=10, return_route=True)
    for excl in (None, sp.csr_matrix((nu, ni), dtype=np.float32),
                 sp.csr_matrix((np.zeros(3, np.float32), (np.array([0, 1, 2]), np.array([4, 5, 6]))), shape=(nu, ni))):
        v, i, r = m.predict_top_k(uf, itf, k=10, return_route=True, exclude=excl)
        assert np.array_equal(v, v0) and np.array_equal(i, i0) and r == r0 and "exclude" not in r


def test_value_errors():
    nu, ni = 50, 300
    m = _model(nu, ni, 16)
    uf, itf = _eye(nu), _eye(ni)
    excl = _excl_matrix(nu, ni, [[1, 2]] * nu)
    with pytest.raises(ValueError):
        m.predict_top_k(uf, itf, k=10, exclude=excl, item_sharded=True)
    with pytest.raises(ValueError):
        m.predict_top_k(uf, itf, k=10, exclude=excl, item_offset=7)
    with pytest.raises(ValueError):
        m.predict_top_k(uf, itf, k=1025, exclude=excl)
    with pytest.raises(ValueError):
        m.predict_top_k(uf, itf, k=10, exclude=sp.csr_matrix((nu + 1, ni)))
    with pytest.raises(ValueError):
        m.predict_top_k(uf, itf, k=10, exclude=sp.csr_matrix((nu, ni + 1)))
    with pytest.raises(ValueError):
        m.predict_rank_of_interactions(uf, itf, sp.csr_matrix((nu, ni)), exclude=sp.csr_matrix((nu, ni + 1)))


def _kernel_case(scores, excl_rows, k):
    s = torch.from_numpy(np.ascontiguousarray(scores, np.float32)).cuda()
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in excl_rows])]).astype(np.int64)
    idx = np.concatenate([np.sort(np.asarray(r, np.int32)) for r in excl_rows] + [np.zeros(0, np.int32)]).astype(np.int32)
    v, i = ops.topk_rows_excluded(s, k, torch.from_numpy(indptr).cuda(), torch.from_numpy(idx).cuda())
    ev, ei = _expected(scores, excl_rows, k)
    assert np.array_equal(i.cpu().numpy(), ei)
    assert np.array_equal(v.cpu().numpy(), ev)


def test_masked_selection_kernel():
    """±inf, -0.0 / +0.0, ties across excluded and non-excluded items, fully excluded rows, k beyond the remaining items, long
    rows with heavy ties (the radix path and its tie-by-index step), a row shorter than k."""
    rng = np.random.default_rng(9)
    n = 3000
    a = rng.standard_normal((8, n)).astype(np.float32)
    a[0, [3, 9, 100]] = np.inf
    a[0, [4, 10]] = -np.inf
    a[1] = np.round(a[1] * 2) / 2                        # few distinct values: ties everywhere
    a[2, :] = -np.inf                                     # every entry -inf: index order
    a[3, ::2] = 0.0
    a[3, 1::2] = -0.0
    a[4] = rng.integers(0, 3, n).astype(np.float32)
    excl = [[3, 5, 9], np.nonzero(a[1] == a[1].max())[0][::2], [0, 1, 2], np.arange(0, n, 3), np.arange(n),   # row 4: all excluded
            np.arange(n - 5), [], rng.choice(n, 100, replace=False)]
    for k in (1, 10, 64, 1000, 1024):
        _kernel_case(a, excl, k)
    long_ties = np.zeros((3, 100_003), np.float32)      # > 4,096 entries reach the floor: radix select, then by index
    long_ties[1, 50_000:] = 1.0
    long_ties[2] = rng.integers(0, 4, 100_003).astype(np.float32)
    lex = [np.arange(0, 100_003, 7), np.arange(50_000, 60_000), rng.choice(100_003, 3000, replace=False)]
    for k in (1, 17, 1024):
        _kernel_case(long_ties, lex, k)
    _kernel_case(a[:, :5], [[1]] * 8, 10)


def _filtered_reference(pred, test, train):
    """(oracle ranks minus the excluded items ahead, at the test pairs) and the masked dense rank matrix"""
    ranks = O.rank_predictions_exact(pred)
    tr = sp.csr_matrix(test)
    rows = np.repeat(np.arange(tr.shape[0]), np.diff(tr.indptr))
    cols = tr.indices
    ex = sp.csr_matrix(train)
    want = np.empty(len(rows), np.int64)
    for p, (u, t) in enumerate(zip(rows, cols)):
        e = ex.indices[ex.indptr[u]:ex.indptr[u + 1]]
        s = pred[u, e]
        want[p] = ranks[u, t] - np.sum((s > pred[u, t]) | ((s == pred[u, t]) & (e < t)))
    masked = pred.copy()
    masked[ex.nonzero()] = -np.inf
    return rows, cols, want, O.rank_predictions_exact(masked)


@pytest.mark.parametrize("n_tastes", [1, 2])
def test_rank_of_interactions_filtered(n_tastes):
    nu, ni = 943, 1682
    m = _model(nu, ni, 64, n_tastes=n_tastes)
    uf, itf = _eye(nu), _eye(ni)
    rng = np.random.default_rng(10 + n_tastes)
    dense = rng.random((nu, ni))
    train = sp.csr_matrix((dense < 0.05).astype(np.float32))
    test = sp.csr_matrix(((dense >= 0.05) & (dense < 0.06)).astype(np.float32))
    pred = m.predict(uf, itf)
    rows, cols, want, masked_ranks = _filtered_reference(pred, test, train)
    pr = m.predict_rank_of_interactions(uf, itf, test, exclude=train)
    assert np.array_equal(pr.rows, rows)
    assert np.array_equal(np.asarray(pr.ranks, np.int64), want)
    for metric in (T.eval.recall_at_k, T.eval.ndcg_at_k):
        assert np.allclose(metric(pr, test, k=10), metric(masked_ranks, test, k=10), equal_nan=True)
    with pytest.raises(ValueError, match="2 test interaction"):
        m.predict_rank_of_interactions(uf, itf, test, exclude=train + _excl_matrix(nu, ni, [list(test[0].indices[:2])] + [[]] * (nu - 1)))
