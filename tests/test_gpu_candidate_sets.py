"""predict_top_k(candidates=...) / predict_rank_of_interactions(candidates=...) on the GPU (docs/candidate_sets.md).  Every expected
value comes from model.predict or ops.pair_scores_exact plus NumPy's lexsort((ids, -vals)); every comparison is an equality."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

import tensorrec_amd as T  # noqa: E402
from tensorrec_amd import candidate_sets as cs, eval as E, ops  # noqa: E402
from tensorrec_amd.prediction_graphs import (CosineSimilarityPredictionGraph, DotProductPredictionGraph,  # noqa: E402
                                             EuclideanSimilarityPredictionGraph)
from tensorrec_amd.representation_graphs import LinearRepresentationGraph  # noqa: E402


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _csr_of(lengths, n_items, rng):
    idx = [np.sort(rng.choice(n_items, int(n), replace=False)).astype(np.int32) for n in lengths]
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return ptr, (np.concatenate(idx) if len(idx) else np.zeros(0, np.int32)).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------ kernel A
@pytest.mark.parametrize("d", [20, 64, 128, 256])
@pytest.mark.parametrize("euclid", [False, True])
@pytest.mark.parametrize("biased", [False, True])
def test_scores_equal_the_exact_pair_chain(d, euclid, biased):
    nu, ni = 97, 3000
    rng = np.random.default_rng(d + 2 * euclid + biased)
    lengths = np.array([(0, 1, 63, 64, 65, 129, 700)[u % 7] for u in range(nu)])
    assert lengths[-1] > 0                                          # the last segment ends exactly at nnz
    ptr, idx = _csr_of(lengths, ni, rng)
    dev = "cuda"
    mode = ops.MODE_EUCLIDEAN if euclid else ops.MODE_DOT
    u_op, u_sq, kpad = ops.score_prep(torch.from_numpy(rng.standard_normal((nu, d)).astype(np.float32)).to(dev), ops.DTYPE_F32,
                                      want_sqnorm=euclid)
    i_op, i_sq, _ = ops.score_prep(torch.from_numpy(rng.standard_normal((ni, d)).astype(np.float32)).to(dev), ops.DTYPE_F32,
                                   want_sqnorm=euclid)
    ub = torch.from_numpy(rng.standard_normal(nu).astype(np.float32)).to(dev) if biased else None
    ib = torch.from_numpy(rng.standard_normal(ni).astype(np.float32)).to(dev) if biased else None
    ptr_d, idx_d = torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)
    seg = np.repeat(np.arange(nu, dtype=np.int32), lengths)
    want = ops.pair_scores_exact(u_op, i_op, kpad, d, torch.from_numpy(seg).to(dev), idx_d, ub, ib, mode, u_sq, i_sq).cpu().numpy()
    got = ops.candset_scores(u_op, i_op, kpad, d, ptr_d, idx_d, len(idx), ub, ib, mode, u_sq, i_sq).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    # rows: user operand row r scores CSR row perm[r]
    perm = rng.permutation(nu).astype(np.int32)
    user_of_seg = np.empty(nu, np.int32)
    user_of_seg[perm] = np.arange(nu, dtype=np.int32)
    want = ops.pair_scores_exact(u_op, i_op, kpad, d, torch.from_numpy(user_of_seg[seg]).to(dev), idx_d, ub, ib, mode, u_sq,
                                 i_sq).cpu().numpy()
    got = ops.candset_scores(u_op, i_op, kpad, d, ptr_d, idx_d, len(idx), ub, ib, mode, u_sq, i_sq,
                             rows=torch.from_numpy(perm).to(dev)).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))


# ------------------------------------------------------------------------------------------------------------ kernel B
def _expected_topk(vals, ids, k):
    o = np.lexsort((ids, -vals))[:k]
    ev = np.full(k, -np.inf, np.float32)
    ei = np.full(k, -1, np.int32)
    ev[:len(o)], ei[:len(o)] = vals[o], ids[o]
    return ev, ei


def _segments(k, rng):
    """Hand-made (values, pattern name) segments: every length with random values, and the value patterns at the lengths where
    they reach both forms."""
    segs = []
    for n in (0, 1, 255, 256, 257, 4096, 4097, 9000):
        segs.append(rng.standard_normal(n).astype(np.float32))
        segs.append(np.full(n, 0.25, np.float32))                                   # all equal: ties broken by id
    for n in (255, 257, 4097, 9000):
        v = rng.standard_normal(n).astype(np.float32)                               # forty equal values straddling place k
        order = np.argsort(-v, kind="stable")
        first = max(0, min(k, n) - 20)
        v[order[first:first + 40]] = v[order[first]]
        segs.append(v)
        z = np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(np.float32)             # +0.0 / -0.0: one key
        z[::7] = -1.0
        segs.append(z)
        w = rng.standard_normal(n).astype(np.float32)                               # -inf entries, more than n - k of them
        w[rng.random(n) < 0.7] = -np.inf
        segs.append(w)
        x = rng.standard_normal(n).astype(np.float32)                               # one NaN: behind -inf
        x[n // 3] = np.nan
        x[n // 2:] = -np.inf
        segs.append(x)
    segs.append(np.full(9000, -3.5, np.float32))                                    # 9,000 equal: the overflow / radix path
    return segs


@pytest.mark.parametrize("k", [1, 10, 64, 300])
def test_segment_topk_against_lexsort(k):
    rng = np.random.default_rng(k)
    segs = _segments(k, rng)
    lengths = np.array([len(s) for s in segs])
    ptr, idx = _csr_of(lengths, 20000, rng)
    vals = np.concatenate(segs).astype(np.float32)
    dev = "cuda"
    lr = cs.long_rows(ptr)
    assert set(lengths[lr]) == {257, 4096, 4097, 9000}
    ov, oi = ops.candset_topk(torch.from_numpy(vals).to(dev), torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev), k,
                              long_rows=torch.from_numpy(lr).to(dev))
    ov, oi = ov.cpu().numpy(), oi.cpu().numpy()
    for r in range(len(segs)):
        ev, ei = _expected_topk(vals[ptr[r]:ptr[r + 1]], idx[ptr[r]:ptr[r + 1]], k)
        assert np.array_equal(oi[r], ei), (r, len(segs[r]))
        assert np.array_equal(_bits(ov[r]), _bits(ev)), (r, len(segs[r]))
    # rows: the call's row r is CSR row perm[r]
    perm = rng.permutation(len(segs)).astype(np.int32)
    lr2 = np.nonzero(lengths[perm] > cs.SHORT_SEGMENT_MAX)[0].astype(np.int32)
    pv, pi = ops.candset_topk(torch.from_numpy(vals).to(dev), torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev), k,
                              long_rows=torch.from_numpy(lr2).to(dev), rows=torch.from_numpy(perm).to(dev))
    assert np.array_equal(pi.cpu().numpy(), oi[perm]) and np.array_equal(_bits(pv.cpu().numpy()), _bits(ov[perm]))


# ------------------------------------------------------------------------------------------------------------ kernel C
def test_rank_count_against_numpy():
    rng = np.random.default_rng(5)
    nu, ni = 40, 500
    lengths = rng.integers(1, 120, size=nu)
    lengths[3] = 0                                                  # a user with no candidates (and two targets)
    ptr, idx = _csr_of(lengths, ni, rng)
    score = rng.integers(-3, 4, size=len(idx)).astype(np.float32)   # few distinct values: many ties
    t_rows, t_idx, t_score = [], [], []
    for u in range(nu):
        if u == 7:
            continue                                                # a user with no targets
        c = idx[ptr[u]:ptr[u + 1]]
        s = score[ptr[u]:ptr[u + 1]]
        inside = rng.choice(len(c), min(2, len(c)), replace=False) if len(c) else []
        for j in inside:                                            # targets stored in the list, with their listed score
            t_rows.append(u), t_idx.append(c[j]), t_score.append(s[j])
        outside = np.setdiff1d(np.arange(ni), c)
        for t in rng.choice(outside, 2, replace=False):             # targets outside it, tied with listed items on both sides
            t_rows.append(u), t_idx.append(t), t_score.append(float(rng.integers(-3, 4)))
    t_rows = np.asarray(t_rows)
    t_idx = np.asarray(t_idx, np.int32)
    t_score = np.asarray(t_score, np.float32)
    pair_ptr = np.searchsorted(t_rows, np.arange(nu + 1)).astype(np.int64)
    dev = "cuda"
    got = ops.candset_rank_count(torch.from_numpy(pair_ptr).to(dev), torch.from_numpy(t_idx).to(dev), torch.from_numpy(t_score).to(dev),
                                 torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev),
                                 torch.from_numpy(score).to(dev)).cpu().numpy()
    want = np.zeros(len(t_idx), np.int32)
    n_tied_below = n_tied_above = 0
    for p, (u, t, st) in enumerate(zip(t_rows, t_idx, t_score)):
        c, s = idx[ptr[u]:ptr[u + 1]], score[ptr[u]:ptr[u + 1]]
        other = c != t
        want[p] = int(np.sum(other & ((s > st) | ((s == st) & (c < t)))))
        n_tied_below += int(np.sum(other & (s == st) & (c < t)))
        n_tied_above += int(np.sum(other & (s == st) & (c > t)))
    assert n_tied_below > 0 and n_tied_above > 0 and pair_ptr[8] == pair_ptr[7] and ptr[4] == ptr[3]
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------ model level
NU, NI = 300, 2000
TIES = [(5, 6), (7, 8), (100, 101)]


def _model(graph, d=64, precision="fp32", **kw):
    m = T.TensorRec(n_components=d, prediction_graph=graph(), user_repr_graph=LinearRepresentationGraph(),
                    item_repr_graph=LinearRepresentationGraph(), seed=0, precision=precision, **kw)
    m.build(NU, NI)
    w = m.get_weights()
    rng = np.random.default_rng(1)
    for name in ("user_feature_biases", "item_feature_biases"):
        w[name] = (0.05 * rng.standard_normal(w[name].shape)).astype(np.float32)
    for a, b in TIES:                                               # identical items: equal scores for every user
        for name in w:
            if name.endswith("item") or name == "item_feature_biases":
                w[name][b] = w[name][a]
    m.set_weights(w)
    return m


def _eye(n):
    return sp.identity(n, dtype=np.float32, format="csr")


def _sets():
    """Per-user candidate lists: 0, 3 (fewer than k), 101 and all 2,000 items, the tied items among them."""
    rng = np.random.default_rng(7)
    per = []
    for u in range(NU):
        n = (0, 3, 101, NI)[u % 4]
        c = rng.choice(NI, n, replace=False)
        if n == 101:
            c = np.unique(np.concatenate([c, np.asarray(TIES[u % 3])]))
        per.append(np.sort(c))
    return per


def _matrix(per):
    rows = np.concatenate([np.full(len(p), u) for u, p in enumerate(per)]).astype(np.int64)
    cols = np.concatenate([np.asarray(p, np.int64) for p in per])
    return sp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(NU, NI))


def _expected_lists(pred, per, k):
    ev = np.full((len(per), k), -np.inf, np.float32)
    ei = np.full((len(per), k), -1, np.int32)
    for u, c in enumerate(per):
        c = np.asarray(c, np.int64)
        ev[u], ei[u] = _expected_topk(pred[u, c], c.astype(np.int32), k)
    return ev, ei


MODELS = [
    (DotProductPredictionGraph, {}, "pairs"),
    (CosineSimilarityPredictionGraph, {}, "pairs"),
    (EuclideanSimilarityPredictionGraph, {}, "pairs"),
    (DotProductPredictionGraph, {"n_tastes": 3}, "slab"),
    (DotProductPredictionGraph, {"precision": "bf16"}, "slab"),
]


@pytest.mark.parametrize("graph,kw,form", MODELS)
def test_top_k_among_candidates(graph, kw, form):
    m = _model(graph, **kw)
    per = _sets()
    pred = m.predict(_eye(NU), _eye(NI))
    vals, idx, rep = m.predict_top_k(_eye(NU), _eye(NI), k=10, candidates=_matrix(per), return_route=True)
    assert rep == m.last_route and rep["route"] == "candidate_sets" and rep["form"] == form and rep["sharded"] is False
    assert rep["k"] == 10 and rep["n_candidates"] == sum(len(p) for p in per) and rep["n_items"] == NI
    assert rep["user_batch_size"] >= 1
    ev, ei = _expected_lists(pred, per, 10)
    assert np.array_equal(idx, ei) and np.array_equal(_bits(vals), _bits(ev))
    # the users who list the whole catalogue: the call without the keyword
    pv, pi = m.predict_top_k(_eye(NU), _eye(NI), k=10)
    full = np.arange(3, NU, 4)
    assert np.array_equal(idx[full], pi[full]) and np.array_equal(_bits(vals[full]), _bits(pv[full]))
    # small user batches give the same lists
    v2, i2 = m.predict_top_k(_eye(NU), _eye(NI), k=10, candidates=_matrix(per), user_batch_size=7)
    assert np.array_equal(i2, idx) and np.array_equal(_bits(v2), _bits(vals))


@pytest.mark.parametrize("graph,kw,form", [MODELS[0], MODELS[3]])
def test_top_k_candidates_minus_exclusions(graph, kw, form):
    m = _model(graph, **kw)
    per = _sets()
    rng = np.random.default_rng(9)
    excl = []
    for u, c in enumerate(per):
        if u % 8 == 2:
            excl.append(np.asarray(c))                              # exclusions that empty the set
        else:
            excl.append(np.unique(np.concatenate([rng.choice(NI, 30, replace=False), c[:len(c) // 3]])))
    left = [np.setdiff1d(c, e) for c, e in zip(per, excl)]
    assert len(per[2]) > 0 and len(left[2]) == 0
    pred = m.predict(_eye(NU), _eye(NI))
    vals, idx, rep = m.predict_top_k(_eye(NU), _eye(NI), k=10, candidates=_matrix(per), exclude=_matrix(excl), return_route=True)
    assert rep["form"] == form and rep["n_candidates"] == sum(len(p) for p in left)
    ev, ei = _expected_lists(pred, left, 10)
    assert np.array_equal(idx, ei) and np.array_equal(_bits(vals), _bits(ev))


def test_no_candidates_is_the_plain_call():
    m = _model(DotProductPredictionGraph)
    v0, i0, r0 = m.predict_top_k(_eye(NU), _eye(NI), k=10, return_route=True)
    plain = dict(m.last_route)
    v1, i1, r1 = m.predict_top_k(_eye(NU), _eye(NI), k=10, return_route=True, candidates=None)
    assert m.last_route == plain and r0 == r1 and np.array_equal(i0, i1) and np.array_equal(_bits(v0), _bits(v1))
    with pytest.raises(ValueError):
        m.predict_top_k(_eye(NU), _eye(NI), k=10, candidates=_matrix(_sets()), item_offset=5)
    with pytest.raises(ValueError):
        m.predict_top_k(_eye(NU), _eye(NI), k=ops.EXCLUDE_K_MAX + 1, candidates=_matrix(_sets()))
    with pytest.raises(ValueError):
        m.predict_top_k(_eye(NU), _eye(NI), k=10, candidates=sp.csr_matrix((NU + 1, NI), dtype=np.float32))


# ------------------------------------------------------------------------------------------------------------ sampled evaluation
@pytest.mark.parametrize("graph,kw,form", [MODELS[0], MODELS[2], MODELS[3], MODELS[4]])
def test_sampled_evaluation(graph, kw, form):
    m = _model(graph, **kw)
    rng = np.random.default_rng(11)
    test_items = [rng.choice(NI, 1 + u % 3, replace=False) for u in range(NU)]
    test_items[4] = np.asarray(TIES[0][:1])
    inter = _matrix(test_items)
    negatives = []
    for u in range(NU):
        neg = rng.choice(np.setdiff1d(np.arange(NI), test_items[u]), 100, replace=False)
        if u == 4:
            neg[0] = TIES[0][1]                                     # a negative tied with the test item
        negatives.append(np.unique(neg))
    pred = m.predict(_eye(NU), _eye(NI))
    r_without = m.predict_rank_of_interactions(_eye(NU), _eye(NI), inter, candidates=_matrix(negatives))
    rows, nth, want = [], [], []
    for u in range(NU):
        c = negatives[u]
        for n, t in enumerate(np.sort(test_items[u])):
            s, st = pred[u, c], pred[u, t]
            rows.append(u)
            nth.append(n)
            want.append(1 + int(np.sum((s > st) | ((s == st) & (c < t)))))
    rows, nth, want = np.asarray(rows), np.asarray(nth), np.asarray(want, np.int32)
    assert np.array_equal(r_without.rows, rows) and np.array_equal(r_without.ranks, want)
    # the test item stored in C_u.  A user's other test items must not be candidates of this one (the rule counts every listed
    # j != t), so pass n ranks every user's n-th test item among its negatives and itself: all pairs are covered once.
    ranks_with = np.zeros_like(want)
    for n in range(3):
        nth_items = [np.sort(t)[n:n + 1] for t in test_items]
        with_test = [np.union1d(neg, t) for neg, t in zip(negatives, nth_items)]
        r = m.predict_rank_of_interactions(_eye(NU), _eye(NI), _matrix(nth_items), candidates=_matrix(with_test))
        assert np.array_equal(r.rows, rows[nth == n])
        ranks_with[nth == n] = r.ranks
    assert np.array_equal(ranks_with, want)
    # all of a user's test items stored at once: each is then a candidate of the others, by the same rule
    every = [np.union1d(neg, t) for neg, t in zip(negatives, test_items)]
    r_every = m.predict_rank_of_interactions(_eye(NU), _eye(NI), inter, candidates=_matrix(every))
    want_every = [1 + int(np.sum((c != t) & ((pred[u, c] > pred[u, t]) | ((pred[u, c] == pred[u, t]) & (c < t)))))
                  for u, c in enumerate(every) for t in np.sort(test_items[u])]
    assert np.array_equal(r_every.rows, rows) and np.array_equal(r_every.ranks, np.asarray(want_every, np.int32))
    r_with = E.PairRanks(rows.astype(np.int32), ranks_with, np.ones(len(want), np.float32), NU)
    expected = E.PairRanks(rows.astype(np.int32), want, np.ones(len(want), np.float32), NU)
    for k in (1, 10):
        assert np.array_equal(E.recall_at_k(r_without, inter, k=k), E.recall_at_k(expected, inter, k=k))
        assert np.array_equal(E.recall_at_k(r_with, inter, k=k), E.recall_at_k(expected, inter, k=k))
