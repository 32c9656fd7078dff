"""tests/warp_reference.py on the CPU: (a) away from the discontinuities the closed-form gradients of the float64 reference are the
central differences of its own loss, the rank weight L held fixed; (b) the float32 restatement of csrc/loss_warp.hip lies inside the
bars on every case the GPU tests run, and the reference alone leaves out (almost) no positive of the real-valued family; the planted
rows hold what they plant; (c) six seeded defects leave the bars or change ``first``; (d) the loss-graph class validates, pickles and
loads a pickle without its attribute, is capturable and has no one-pass route; (e) the two entry points refuse bad arguments before
any launch."""
import ctypes
import functools
import pickle

import numpy as np
import pytest

import warp_reference as W
from sampled_loss_reference import f64


# ------------------------------------------------------------------------------------------------ (a) closed forms
def small_case(remove_hits):
    rng = np.random.default_rng(5)
    indptr = np.array([0, 4, 6, 11], dtype=np.int64)
    values = np.array([1.0, -1.0, 2.0, 0.5, 0.0, -2.0, 1.0, 1.0, 0.0, 3.0, 1.0], dtype=np.float32)     # user 1: non-positives only
    x_item = np.array([0, 2, 5, 7, 1, 3, 0, 1, 4, 6, 8], dtype=np.int32)
    samples = np.array([[5, 9, 9, 2, 3, 7], [1, 2, 3, 4, 5, 6], [6, 4, 2, 9, 0, 3]], dtype=np.int32)
    pred, samp = rng.standard_normal(11), rng.standard_normal((3, 6))
    go = rng.uniform(0.5, 1.5, int((values > 0).sum())) * np.array([1, -1, 1, 1, -1, 1, 1])
    go[2] = 0.0
    return indptr, values, pred, samp, go, samples, x_item


@pytest.mark.parametrize("remove_hits", [False, True])
def test_reference_gradients_are_central_differences(remove_hits):
    indptr, values, pred, samp, go, samples, x_item = small_case(remove_hits)
    fn = lambda p, s: W.ref_warp(indptr, values, p, s, go, 40, samples, x_item, remove_hits)
    ref = fn(pred, samp)
    h = 1e-4

    def total(p, s):
        r = fn(p, s)
        assert np.array_equal(r.first, ref.first) and np.array_equal(r.weight, ref.weight)        # no discontinuity crossed: L is fixed
        return float((go * r.loss).sum())
    fd_p, fd_s = np.zeros_like(pred), np.zeros_like(samp)
    for i in range(pred.size):
        d = np.zeros_like(pred)
        d[i] = h
        fd_p[i] = (total(pred + d, samp) - total(pred - d, samp)) / (2 * h)
    for i in range(samp.size):
        d = np.zeros(samp.size)
        d[i] = h
        d = d.reshape(samp.shape)
        fd_s[i // samp.shape[1], i % samp.shape[1]] = (total(pred, samp + d) - total(pred, samp - d)) / (2 * h)
    assert np.abs(fd_p - ref.d_pred).max() <= 1e-9 * np.abs(ref.d_pred).max()
    assert np.abs(fd_s - ref.d_samp).max() <= 1e-9 * np.abs(ref.d_samp).max()
    assert (ref.d_pred[values <= 0] == 0).all() and (ref.d_samp[1] == 0).all() and ref.d_samp[0].any()
    assert (ref.first[values <= 0] == -1).all() and (ref.first[values > 0] >= 0).any()
    if remove_hits:
        plain = W.ref_warp(indptr, values, pred, samp, go, 40)
        assert (ref.trials < ref.first + 1).any() or not np.array_equal(ref.first, plain.first)   # the mask bites


# ------------------------------------------------------------------------------------------------ (b) the restatement, the cases
@functools.lru_cache(maxsize=None)
def cached(family, *key):
    case = {"real": W.real_case, "dyadic": W.dyadic_case, "planted": W.planted_case, "hits": W.hits_case}[family](*key)
    return case, W.run_ref(case, remove_hits=family == "hits")


def outside(case, got, ref, exact_first):
    """per output (loss, d_pred, d_samp): does a compared entry lie outside its bar?  and: does ``first`` differ where it is compared?"""
    loss, first, d_pred, d_samp = got
    keep_pos, keep_p, rows, left_out = W.comparable(case, ref)
    if exact_first:
        keep_pos, keep_p, rows = np.ones_like(keep_pos), np.ones_like(keep_p), np.ones_like(rows)
    out = [bool((np.abs(f64(loss) - ref.loss) > ref.bar_loss)[keep_pos].any()),
           bool((np.abs(f64(d_pred) - ref.d_pred) > ref.bar_d_pred)[keep_p].any()),
           bool((np.abs(f64(d_samp) - ref.d_samp) > ref.bar_d_samp)[rows].any())]
    return out, bool((first != ref.first)[keep_p].any()), left_out


ALL_REAL = sorted(set(W.SAMPLE_COUNTS + W.SAMPLE_COUNTS_MANY))


@pytest.mark.parametrize("S", ALL_REAL)
def test_real_family_restatement_and_the_share_left_out(S):
    case, ref = cached("real", S)
    assert not (case.pred * 1024 == np.round(case.pred * 1024)).all() and (case.go < 0).any() and (case.go > 0).any() \
        and (case.go == 0).any()
    out, first_differs, left_out = outside(case, W.f32_warp(case), ref, False)
    assert out == [False] * 3 and not first_differs
    # about 2e-7 per scanned cell: the reference alone leaves out essentially none
    assert left_out <= W.MAX_LEFT_OUT and ref.near.sum() <= max(1, 1e-5 * ref.scanned), (int(ref.near.sum()), ref.scanned)
    assert all(np.isfinite(x).all() and (x >= 0).all() for x in W.bars(ref))
    slot = np.cumsum(case.values > 0) - 1
    assert ref.first[case.planted.far_above] == -1 and ref.loss[slot[case.planted.far_above]] == 0
    assert ref.first[case.planted.far_below] == 0 and ref.loss[slot[case.planted.far_below]] > 100
    u5 = ref.first[case.indptr[5]:case.indptr[6]]
    assert set(u5.tolist()) <= {-1, 0}                                  # equal samples: the lowest index or none


@pytest.mark.parametrize("S", ALL_REAL)
def test_dyadic_family_restatement(S):
    case, ref = cached("dyadic", S)
    assert W.values_exact(case)
    got = W.f32_warp(case)
    out, first_differs, _ = outside(case, got, ref, True)
    assert out == [False] * 3 and not first_differs
    for g, want in zip((got[0], got[2], got[3]), (ref.loss, ref.d_pred, ref.d_samp)):
        assert np.array_equal(g == 0, want == 0)


@pytest.mark.parametrize("S,n_items,firsts", W.PLANTED, ids=["%d-%d" % p[:2] for p in W.PLANTED])
def test_planted_rows_hold_what_they_plant(S, n_items, firsts):
    case, ref = cached("planted", S, n_items, tuple(firsts))
    assert case.names[:2] == ["empty", "non-positive"] and case.indptr[1] == 0 and not (case.values[:2] > 0).any()
    for p, want in case.expected.items():
        assert ref.first[p] == want, (p, want, ref.first[p])
    assert sorted(set(k for k in ref.first if k > 0)) == sorted(set(k for k in firsts if k > 0) | ({1} if S > 1 else set()))
    got = W.f32_warp(case)
    out, first_differs, _ = outside(case, got, ref, True)
    assert out == [False] * 3 and not first_differs
    stopped = ref.first >= 0
    if S == 2000:
        dead = stopped & (ref.trials >= 1350)
        assert dead.sum() >= 4 and (ref.weight[dead] == 0).all() and (ref.d_pred[dead] == 0).all()
        assert np.isclose(ref.weight[ref.trials == 1349], np.log(2.0)).all() and (ref.trials == 1349).sum() == 2
    if n_items == 50:
        assert (stopped & (ref.trials > n_items - 1)).sum() >= 4 and (ref.weight[stopped & (ref.trials >= 49)] == 0).all()
        assert (ref.weight[stopped & (ref.trials == 1)] == np.log(49.0)).all()
    assert (ref.d_samp[:2] == 0).all() and ref.d_samp.any()
    ref_h = W.run_ref(case, remove_hits=True)                             # a hit one slot before the violator: the same first, N - 1
    late = ref.first > 1                                                  # (first = 1 is the zero / eps row, which holds no hit)
    assert np.array_equal(ref_h.first, ref.first) and np.array_equal(ref_h.trials[late], ref.trials[late] - 1)
    assert np.array_equal(ref_h.trials[~late], ref.trials[~late]) and (late.any() or S == 1)
    out, first_differs, _ = outside(case, W.f32_warp(case, remove_hits=True), ref_h, True)
    assert out == [False] * 3 and not first_differs


@pytest.mark.parametrize("S", W.SAMPLE_COUNTS + [40])
def test_hit_removal_cases(S):
    case, ref = cached("hits", S)
    plain = W.run_ref(case, remove_hits=False)
    assert W.values_exact(case)
    rows = lambda r, u: r[case.indptr[u]:case.indptr[u + 1]]
    pos = lambda u: rows(case.values, u) > 0
    assert (rows(ref.first, W.U_ALL_HITS) == -1).all() and (ref.d_samp[W.U_ALL_HITS] == 0).all() and \
        (rows(plain.first, W.U_ALL_HITS) >= 0).any()
    assert (rows(ref.first, W.U_ONLY_HIT) == -1).all() and rows(plain.first, W.U_ONLY_HIT)[pos(W.U_ONLY_HIT)].tolist() == [case.k7]
    for u, n in ((W.U_HIT_FIRST, 3), (W.U_LONG, 5)):
        f, t = rows(ref.first, u)[pos(u)][:n], rows(ref.trials, u)[pos(u)][:n]
        assert (f == 1).all() and (t == 1).all() if S > 1 else (f == -1).all()
    assert (np.diff(case.indptr)[[W.U_HIT_FIRST, W.U_NON_POSITIVE, W.U_ONLY_HIT]] <= 64).all() and np.diff(case.indptr)[W.U_LONG] > 64
    f5 = rows(ref.first, W.U_NON_POSITIVE)[pos(W.U_NON_POSITIVE)]
    assert (f5 == 0).all()                                                # the column of a non-positive interaction is no hit
    if S >= 4:
        ids = case.samples[W.U_NON_POSITIVE]
        assert ids[1] == ids[2] and ids[3] == ids[0]
    assert any(np.unique(row).size < row.size for row in case.samples) or S == 1
    if S > 1:
        assert ((ref.first >= 0) & (ref.trials < ref.first + 1)).sum() >= 8        # a hit in front of the violator: N drops
    got = W.f32_warp(case, remove_hits=True)
    out, first_differs, _ = outside(case, got, ref, True)
    assert out == [False] * 3 and not first_differs
    for g, want in zip((got[0], got[2], got[3]), (ref.loss, ref.d_pred, ref.d_samp)):
        assert np.array_equal(g == 0, want == 0)


# ------------------------------------------------------------------------------------------------ (c) seeded defects
@pytest.mark.parametrize("defect", W.DEFECTS)
def test_seeded_defects_are_caught(defect):
    assert len(W.DEFECTS) >= 6
    caught = 0
    for family, key in (("planted", W.PLANTED[3]), ("planted", W.PLANTED[-1]), ("dyadic", (65,)), ("hits", (65,))):
        key = (key[0], key[1], tuple(key[2])) if family == "planted" else key
        case, ref = cached(family, *key)
        out, first_differs, _ = outside(case, W.f32_warp(case, remove_hits=family == "hits", defect=defect), ref, True)
        caught += any(out) or first_differs
    assert caught >= 1, defect


# ------------------------------------------------------------------------------------------------ (d) the class
def test_loss_graph_class_validates_pickles_and_routes():
    from tensorrec_amd.loss_graphs import WARPLossGraph, WMRBLossGraph
    import tensorrec_amd.tensorrec as TT
    from tensorrec_amd import ops, step_plan
    g = WARPLossGraph()
    assert g.remove_accidental_hits is False and g.wants_sample_items is False
    h = pickle.loads(pickle.dumps(WARPLossGraph(remove_accidental_hits=True)))
    assert isinstance(h, WARPLossGraph) and h.remove_accidental_hits is True and h.wants_sample_items is True
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError):
            WARPLossGraph(bad)
    assert WARPLossGraph.is_sample_based is True and WARPLossGraph.is_sampled_with_replacement is False and WARPLossGraph.is_dense is False
    old = WARPLossGraph()
    old.__dict__.clear()                                                  # a pickle from before the attribute existed
    old = pickle.loads(pickle.dumps(old))
    assert old.__dict__ == {} and old.remove_accidental_hits is False and old.wants_sample_items is False
    assert WARPLossGraph in TT._GRAPH_CAPTURABLE_LOSSES
    assert step_plan.loss_kind(WARPLossGraph()) is None and step_plan.loss_kind(WARPLossGraph(True)) is None
    assert step_plan.loss_kind(WMRBLossGraph()) is not None
    assert callable(ops.warp_loss)


# ------------------------------------------------------------------------------------------------ (e) the entry points
def test_entry_points_refuse_bad_arguments_before_any_launch():
    from tensorrec_amd import _native
    lib = _native.load()
    p = ctypes.c_void_p(8)

    def fwd(S=5, n_items=2700, first=p, x_item=None, samples=None, hits=0, n_users=1, last=p):
        return lib.trec_warp_fwd(first, x_item, p, p, p, samples, n_users, n_items, S, hits, p, p, last, None)

    def bwd(S=5, first=p, n_users=1, last=p):
        return lib.trec_warp_bwd(first, p, p, p, p, n_users, S, p, last, None)

    for name, fn in (("trec_warp_fwd", fwd), ("trec_warp_bwd", bwd)):
        for kw in ({"first": None}, {"last": None}):
            assert fn(**kw) == 1
            assert lib.trec_last_error() == (name + ": null pointer").encode()
        for S in (0, -1, 16385):
            assert fn(S=S) == 1
            assert lib.trec_last_error() == (name + ": n_sampled must be in [1, 16384]").encode()
        assert fn(n_users=0) == 0                                         # nothing to do, no launch
    for n_items in (0, -3, 2 ** 31, 2 ** 40):
        assert fwd(n_items=n_items) == 1
        assert lib.trec_last_error() == b"trec_warp_fwd: n_items must be in [1, 2^31)"
    assert fwd(hits=1, x_item=p) == 1 and lib.trec_last_error() == b"trec_warp_fwd: null samples with remove_hits"
    assert fwd(hits=1, samples=p) == 1 and lib.trec_last_error() == b"trec_warp_fwd: null x_item with remove_hits"
    assert fwd(n_users=0, n_items=2 ** 31 - 1, S=16384) == 0 and fwd(n_users=0, hits=1, x_item=p, samples=p) == 0
    # every other required pointer, one at a time
    args = [p, None, p, p, p, None, 1, 2700, 5, 0, p, p, p, None]
    for k in (2, 3, 4, 10, 11, 12):
        a = list(args)
        a[k] = None
        assert lib.trec_warp_fwd(*a) == 1
    args = [p, p, p, p, p, 1, 5, p, p, None]
    for k in (0, 1, 2, 3, 4, 7, 8):
        a = list(args)
        a[k] = None
        assert lib.trec_warp_bwd(*a) == 1
