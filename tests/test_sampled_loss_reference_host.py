"""tests/sampled_loss_reference.py on the CPU: (a) the closed-form gradients of the float64 references are the central differences of
their own losses; (b) float32 NumPy restatements of the formulas of csrc/loss_sampled.hip, on every case the GPU tests run and with
the sums taken in two orders, lie inside the bars; (c) seeded defects leave them; (d) the loss-graph classes validate and pickle;
(e) the four entry points refuse bad arguments before any launch."""
import ctypes
import functools
import pickle

import numpy as np
import pytest

import sampled_loss_reference as R
from sampled_loss_reference import f64

F = np.float32


# ------------------------------------------------------------------------------------------------ (a) closed forms
def small_case():
    rng = np.random.default_rng(5)
    indptr = np.array([0, 4, 6, 11], dtype=np.int64)
    values = np.array([1.0, -1.0, 2.0, 0.5, 0.0, -2.0, 1.0, 1.0, 0.0, 3.0, 1.0], dtype=np.float32)     # user 1: non-positives only
    pred, samp = rng.standard_normal(11), rng.standard_normal((3, 6))
    go = rng.uniform(0.5, 1.5, int((values > 0).sum()))
    go[2] = 0.0
    return indptr, values, pred, samp, go


@pytest.mark.parametrize("name", ["softmax-1", "softmax-0.25", "bpr"])
def test_reference_gradients_are_central_differences(name):
    indptr, values, pred, samp, go = small_case()
    if name == "bpr":
        fn = lambda p, s: R.ref_bpr(indptr, values, p, s, go)
    else:
        fn = lambda p, s: R.ref_sampled_softmax(indptr, values, p, s, go, float(name.split("-")[1]))
    ref = fn(pred, samp)
    total = lambda p, s: float((go * fn(p, s).loss).sum())
    h = 1e-5
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
    assert np.abs(fd_p - ref.d_pred).max() <= 1e-6 * np.abs(ref.d_pred).max()
    assert np.abs(fd_s - ref.d_samp).max() <= 1e-6 * np.abs(ref.d_samp).max()
    assert (ref.d_pred[values <= 0] == 0).all() and (ref.d_samp[1] == 0).all() and ref.d_samp[0].any()


# ------------------------------------------------------------------------------------------------ (b) float32 restatements
def fsum(x, order, axis=-1):
    """float32 sums in two orders: NumPy's pairwise sum, and a sequential chain from the far end"""
    x = np.asarray(x, dtype=F)
    if order == 0:
        return np.sum(x, axis=axis, dtype=F)
    return np.take(np.cumsum(np.flip(x, axis=axis), axis=axis, dtype=F), -1, axis=axis)


def f32_sampled_softmax(case, temperature, order, defect=None):
    """csrc/loss_sampled.hip's sampled softmax, every operation in float32"""
    t = F(1.0 / temperature)
    pos = case.values > 0 if defect != "count_non_positives" else np.ones(case.values.size, bool)
    true_pos = case.values > 0
    slot = np.cumsum(true_pos) - 1
    loss, d_pred, d_samp = np.zeros(int(true_pos.sum()), F), np.zeros(case.pred.size, F), np.zeros(case.samp.shape, F)
    with np.errstate(over="ignore", invalid="ignore"):
        for u in range(case.n_users):
            idx = np.arange(case.indptr[u], case.indptr[u + 1])
            idx = idx[pos[idx]]
            if not idx.size:
                continue
            ys = case.samp[u]
            M = ys.max()
            E = np.exp((ys - M) * t)
            Z = fsum(np.exp(ys * t), order) if defect == "no_shift" else fsum(E, order)
            yp = case.pred[idx]
            g = np.where(true_pos[idx], case.go[np.maximum(slot[idx], 0)], F(1.0)).astype(F)
            m = np.full_like(yp, M) if defect == "m_is_M" else np.maximum(M, yp)
            a, b = np.exp((yp - m) * t), np.exp((M - m) * t)
            bz = b * Z
            D = a + bz
            lo = (m - yp) * t + np.log(D)
            loss[slot[idx][true_pos[idx]]] = lo[true_pos[idx]]
            d_pred[idx] = -(g * t) * (bz / D)
            K = fsum((g * b) / D, order)
            d_samp[u] = E * K if defect == "no_t" else (t * E) * K
    return loss, d_pred, d_samp


def f32_bpr(case, order, defect=None):
    pos = case.values > 0
    slot = np.cumsum(pos) - 1
    S = case.S
    inv_s = F(1.0) if defect == "no_inv_s" else F(1.0) / F(S)
    loss, d_pred, d_samp = np.zeros(int(pos.sum()), F), np.zeros(case.pred.size, F), np.zeros(case.samp.shape, F)
    for u in range(case.n_users):
        idx = np.arange(case.indptr[u], case.indptr[u + 1])
        idx = idx[pos[idx]]
        if not idx.size:
            continue
        yp, g = case.pred[idx], case.go[slot[idx]]
        X = case.samp[u][None, :] - yp[:, None]
        e = np.exp(-np.abs(X))
        spl = np.maximum(X, F(0)) + np.log1p(e)
        loss[slot[idx]] = fsum(spl, order, axis=1) * inv_s
        sig = np.where(X >= 0, F(1), e) / (F(1) + e)
        if defect == "one_minus_sigma":
            sig = F(1) - sig
        c = g * inv_s
        d_pred[idx] = -c * fsum(sig, order, axis=1)
        d_samp[u] = fsum(c[:, None] * sig, order, axis=0)
    return loss, d_pred, d_samp


ALL_S = sorted(set(R.SAMPLE_COUNTS + R.SAMPLE_COUNTS_MANY))


@functools.lru_cache(maxsize=None)
def cached_case(S):
    return R.loss_case(S)


@functools.lru_cache(maxsize=None)
def cached_ref(name, S):
    case = cached_case(S)
    if name == "bpr":
        return R.ref_bpr(case.indptr, case.values, case.pred, case.samp, case.go)
    return R.ref_sampled_softmax(case.indptr, case.values, case.pred, case.samp, case.go, float(name))


def outside(got, ref):
    """per output: does any entry lie outside its bar (or is not finite)?"""
    out = []
    for g, want, bar in zip(got, (ref.loss, ref.d_pred, ref.d_samp), R.bars(ref)):
        g = f64(g)
        out.append(bool((~np.isfinite(g)).any() or (np.abs(g - want) > bar).any()))
    return out


def worst(got, ref):
    return [float(np.max(np.abs(f64(g) - want) / np.maximum(bar, 1e-300), initial=0.0) if np.isfinite(f64(g)).all() else np.inf)
            for g, want, bar in zip(got, (ref.loss, ref.d_pred, ref.d_samp), R.bars(ref))]


@pytest.mark.parametrize("S", ALL_S)
def test_case_holds_what_the_issue_plants(S):
    case = cached_case(S)
    p = R.case_properties(case)
    assert p["positives"] == R.POSITIVES and p["interactions_user1"] == 3 and p["negatives"] > 20 and p["zeros"] > 20
    assert p["above"] and p["equal"] and p["below"] and p["all_equal"]
    assert abs(p["far_above"] - 100.0) < 1e-4 and abs(p["far_below"] - 100.0) < 1e-4 and (S == 1 or p["span"] == 60.0)
    assert p["go_zeros"] >= 100 and p["go_distinct"] > 1000
    assert not (case.pred * 1024 == np.round(case.pred * 1024)).all()                # real-valued, not dyadic
    for temperature in R.TEMPERATURES:
        ref = cached_ref(temperature, S)
        assert all(np.isfinite(x).all() for x in (ref.loss, ref.d_pred, ref.d_samp) + R.bars(ref))
        assert all((b >= 0).all() for b in R.bars(ref)) and (ref.bar_loss >= R.U32).all()
        slot = np.cumsum(case.values > 0) - 1
        assert ref.loss[slot[case.planted.far_above]] < 1e-38 and ref.loss[slot[case.planted.far_below]] >= 99.99 / temperature


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("S", ALL_S)
def test_float32_restatements_lie_inside_the_bars(S, order):
    case = cached_case(S)
    for temperature in R.TEMPERATURES:
        got = f32_sampled_softmax(case, temperature, order)
        assert outside(got, cached_ref(temperature, S)) == [False] * 3, ("softmax", temperature, worst(got, cached_ref(temperature, S)))
    got = f32_bpr(case, order)
    assert outside(got, cached_ref("bpr", S)) == [False] * 3, ("bpr", worst(got, cached_ref("bpr", S)))


# ------------------------------------------------------------------------------------------------ (c) seeded defects
@pytest.mark.parametrize("defect", ["no_t", "m_is_M", "no_shift", "count_non_positives"])
def test_softmax_defects_leave_the_bars(defect):
    hits = 0
    for S in (1, 65, 300):
        case = cached_case(S)
        for temperature in R.TEMPERATURES:
            hits += any(outside(f32_sampled_softmax(case, temperature, 0, defect), cached_ref(temperature, S)))
    assert hits >= 1, defect


@pytest.mark.parametrize("defect", ["one_minus_sigma", "no_inv_s"])
def test_bpr_defects_leave_the_bars(defect):
    hits = sum(any(outside(f32_bpr(cached_case(S), 0, defect), cached_ref("bpr", S))) for S in (1, 65, 300))
    assert hits >= 1, defect


# ------------------------------------------------------------------------------------------------ (d) the classes
def test_loss_graph_classes_validate_and_pickle():
    from tensorrec_amd.loss_graphs import SampledSoftmaxLossGraph, BPRLossGraph
    g = pickle.loads(pickle.dumps(SampledSoftmaxLossGraph(0.5)))
    assert isinstance(g, SampledSoftmaxLossGraph) and g.temperature == 0.5
    assert SampledSoftmaxLossGraph().temperature == 1.0
    assert isinstance(pickle.loads(pickle.dumps(BPRLossGraph())), BPRLossGraph)
    for cls in (SampledSoftmaxLossGraph, BPRLossGraph):
        assert cls.is_sample_based is True and cls.is_sampled_with_replacement is False and cls.is_dense is False
    for bad in (0, -1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            SampledSoftmaxLossGraph(bad)
    import tensorrec_amd.tensorrec as TT
    from tensorrec_amd import ops
    assert SampledSoftmaxLossGraph in TT._GRAPH_CAPTURABLE_LOSSES and BPRLossGraph in TT._GRAPH_CAPTURABLE_LOSSES
    assert callable(ops.sampled_softmax_loss) and callable(ops.bpr_loss)


# ------------------------------------------------------------------------------------------------ (e) the entry points
def test_entry_points_refuse_bad_arguments_before_any_launch():
    from tensorrec_amd import _native
    lib = _native.load()
    p = ctypes.c_void_p(8)

    def softmax_fwd(S=5, t=1.0, first=p):
        return lib.trec_sampled_softmax_fwd(first, p, p, p, 1, S, t, p, p, p, None)

    def softmax_bwd(S=5, t=1.0, first=p):
        return lib.trec_sampled_softmax_bwd(first, p, p, p, p, p, p, 1, S, t, p, p, None)

    def bpr_fwd(S=5, first=p):
        return lib.trec_bpr_fwd(first, p, p, p, 1, S, p, None)

    def bpr_bwd(S=5, first=p):
        return lib.trec_bpr_bwd(first, p, p, p, p, 1, S, p, p, None)

    for name, fn in (("trec_sampled_softmax_fwd", softmax_fwd), ("trec_sampled_softmax_bwd", softmax_bwd), ("trec_bpr_fwd", bpr_fwd),
                     ("trec_bpr_bwd", bpr_bwd)):
        assert fn(first=None) == 1
        assert lib.trec_last_error() == (name + ": null pointer").encode()
        for S in (0, 16385):
            assert fn(S=S) == 1
            assert lib.trec_last_error() == (name + ": n_sampled must be in [1, 16384]").encode()
    for name, fn in (("trec_sampled_softmax_fwd", softmax_fwd), ("trec_sampled_softmax_bwd", softmax_bwd)):
        for t in (0.0, -1.0, float("nan"), float("inf")):
            assert fn(t=t) == 1
            assert lib.trec_last_error() == (name + ": inv_temperature must be finite and > 0").encode()
    # every other pointer, one at a time
    assert lib.trec_sampled_softmax_fwd(p, p, p, p, 1, 5, 1.0, p, p, None, None) == 1
    assert lib.trec_sampled_softmax_bwd(p, p, p, p, p, None, p, 1, 5, 1.0, p, p, None) == 1
    assert lib.trec_bpr_fwd(p, p, p, p, 1, 5, None, None) == 1
    assert lib.trec_bpr_bwd(p, p, p, p, p, 1, 5, p, None, None) == 1
    # n_users == 0: nothing to do, no launch
    assert lib.trec_sampled_softmax_fwd(p, p, p, p, 0, 5, 1.0, p, p, p, None) == 0
    assert lib.trec_sampled_softmax_bwd(p, p, p, p, p, p, p, 0, 5, 1.0, p, p, None) == 0
    assert lib.trec_bpr_fwd(p, p, p, p, 0, 5, p, None) == 0 and lib.trec_bpr_bwd(p, p, p, p, p, 0, 5, p, p, None) == 0
