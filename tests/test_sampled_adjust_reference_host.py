"""tests/sampled_adjust_reference.py on the CPU: (a) the closed-form gradients of the float64 references are the central differences of
their own losses, and the references with the options off are those of tests/sampled_loss_reference.py; (b) float32 NumPy restatements
of the adjusted kernels of csrc/loss_sampled.hip, on every case the GPU tests run and with the sums taken in two orders, lie inside the
bars; (c) seeded defects leave them; (d) the cases hold what they claim to plant; (e) the entry points refuse bad arguments."""
import ctypes
import functools

import numpy as np
import pytest

import sampled_adjust_reference as R
import sampled_loss_reference as R0
from sampled_loss_reference import f64
from test_sampled_loss_reference_host import fsum, outside, worst

F = np.float32


# ------------------------------------------------------------------------------------------------ (a) closed forms
@functools.lru_cache(maxsize=None)
def cached_case(S):
    return R.adjust_case(S)


@functools.lru_cache(maxsize=None)
def cached_ref(name, S, temperature=None):
    case = cached_case(S)
    if name == "bpr":
        return R.ref_bpr_adj(case)
    use_q, no_hits, log_q = R.CONFIGS[name]
    return R.ref_sampled_softmax_adj(case, temperature, use_q, no_hits, log_q)


def small_case():
    """the users of adjust_case(6) with at most 65 interactions, so that central differences stay cheap"""
    import copy
    case = copy.copy(cached_case(6))
    case.pred, case.samp, case.go = f64(case.pred), f64(case.samp), f64(case.go)
    return case


@pytest.mark.parametrize("name", ["logq-1", "hits-0.25", "both-0.25", "both-uniform-1", "bpr"])
def test_reference_gradients_are_central_differences(name):
    import copy
    case = small_case()
    if name == "bpr":
        fn = lambda c: R.ref_bpr_adj(c)
    else:
        config, temperature = name.rsplit("-", 1)
        use_q, no_hits, log_q = R.CONFIGS[config]
        fn = lambda c: R.ref_sampled_softmax_adj(c, float(temperature), use_q, no_hits, log_q)
    ref = fn(case)

    def total(pred=None, samp=None):
        c = copy.copy(case)
        c.pred = case.pred if pred is None else pred
        c.samp = case.samp if samp is None else samp
        return float((case.go * fn(c).loss).sum())
    h = 1e-5
    small = [u for u in range(case.n_users) if case.indptr[u + 1] - case.indptr[u] <= 70]
    for u in small:
        for p in range(case.indptr[u], case.indptr[u + 1], 7):
            d = np.zeros(case.pred.size)
            d[p] = h
            fd = (total(pred=case.pred + d) - total(pred=case.pred - d)) / (2 * h)
            assert abs(fd - ref.d_pred[p]) <= 1e-6 * max(1.0, np.abs(ref.d_pred).max()), (u, p)
        for s in range(case.S):
            d = np.zeros(case.samp.shape)
            d[u, s] = h
            fd = (total(samp=case.samp + d) - total(samp=case.samp - d)) / (2 * h)
            assert abs(fd - ref.d_samp[u, s]) <= 1e-6 * max(1.0, np.abs(ref.d_samp).max()), (u, s)
    assert (ref.d_pred[case.values <= 0] == 0).all() and (ref.d_samp[:2] == 0).all()
    if name != "logq-1":
        assert (ref.d_samp[ref.hits] == 0).all() and (ref.d_samp[R.U_ALL_HITS] == 0).all()


@pytest.mark.parametrize("S", [1, 65])
def test_options_off_is_the_plain_reference(S):
    case = cached_case(S)
    for temperature in R.TEMPERATURES:
        a = R.ref_sampled_softmax_adj(case, temperature, False, False)
        b = R0.ref_sampled_softmax(case.indptr, case.values, case.pred, case.samp, case.go, temperature)
        for x, y in ((a.loss, b.loss), (a.d_pred, b.d_pred), (a.d_samp, b.d_samp)):
            assert np.allclose(x, y, rtol=1e-12, atol=1e-300)
    a, b = R.ref_bpr_adj(case, remove_hits=False), R0.ref_bpr(case.indptr, case.values, case.pred, case.samp, case.go)
    for x, y in ((a.loss, b.loss), (a.d_pred, b.d_pred), (a.d_samp, b.d_samp), (a.bar_loss, b.bar_loss), (a.bar_d_samp, b.bar_d_samp)):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------ (b) float32 restatements
def f32_softmax_adj(case, temperature, use_q, no_hits, log_q, order, defect=None):
    """the adjusted sampled softmax of csrc/loss_sampled.hip, every operation in float32"""
    t = F(1.0 / temperature)
    S = case.S
    true_pos = case.values > 0
    slot = np.cumsum(true_pos) - 1
    hits = np.zeros(case.samp.shape, bool)
    if no_hits and defect != "hit_as_negative":
        hits = R.hit_mask(case.indptr, case.cols, case.values, case.items, count_non_positives=defect == "non_positive_is_hit")
    log_s = F(0.0) if defect == "no_log_s" else F(np.log(float(S)))

    def corr(items):
        lq = log_q[items] if log_q is not None else np.full(np.shape(items), F(-np.log(float(case.n_items))))
        return -(log_s + lq.astype(F)) if use_q else np.zeros(np.shape(items), F)
    loss, d_pred, d_samp = np.zeros(int(true_pos.sum()), F), np.zeros(case.pred.size, F), np.zeros(case.samp.shape, F)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for u in range(case.n_users):
            idx = np.arange(case.indptr[u], case.indptr[u + 1])
            idx = idx[true_pos[idx]]
            kept = ~hits[u]
            if not idx.size or not kept.any():
                continue
            ys, c = case.samp[u], corr(case.items[u])
            over = np.ones(S, bool) if defect == "max_over_masked" else kept
            Rm = ys[over].max()
            w = (ys - Rm) * t + c
            M = w[over].max()
            E = np.where(kept, np.exp(w - M), F(0))
            Z = fsum(E, order)
            yp, g = case.pred[idx], case.go[slot[idx]]
            wp = (yp - Rm) * t
            if defect == "c_on_positive":
                wp = wp + corr(case.cols[idx])
            m = np.maximum(M, wp)
            a, b = np.exp(wp - m), np.exp(M - m)
            bz = b * Z
            D = a + bz
            loss[slot[idx]] = (m - wp) + np.log(D)
            d_pred[idx] = -(g * t) * (bz / D)
            K = fsum((g * b) / D, order)
            d_samp[u] = (t * E) * K
    return loss, d_pred, d_samp


def f32_bpr_adj(case, order, defect=None):
    pos = case.values > 0
    slot = np.cumsum(pos) - 1
    hits = R.hit_mask(case.indptr, case.cols, case.values, case.items)
    loss, d_pred, d_samp = np.zeros(int(pos.sum()), F), np.zeros(case.pred.size, F), np.zeros(case.samp.shape, F)
    for u in range(case.n_users):
        idx = np.arange(case.indptr[u], case.indptr[u + 1])
        idx = idx[pos[idx]]
        kept = ~hits[u]
        if not idx.size or not kept.any():
            continue
        inv_s = F(1.0) / F(kept.sum() if defect == "kept_count" else case.S)
        yp, g = case.pred[idx], case.go[slot[idx]]
        X = case.samp[u][kept][None, :] - yp[:, None]
        e = np.exp(-np.abs(X))
        spl = np.maximum(X, F(0)) + np.log1p(e)
        loss[slot[idx]] = fsum(spl, order, axis=1) * inv_s
        sig = np.where(X >= 0, F(1), e) / (F(1) + e)
        c = g * inv_s
        d_pred[idx] = -c * fsum(sig, order, axis=1)
        d_samp[u, kept] = fsum(c[:, None] * sig, order, axis=0)
    return loss, d_pred, d_samp


def f32_config(case, name, temperature, order, defect=None):
    use_q, no_hits, log_q = R.CONFIGS[name]
    return f32_softmax_adj(case, temperature, use_q, no_hits, case.log_q if log_q == "case" else None, order, defect)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("S", R.SAMPLE_COUNTS)
def test_float32_restatements_lie_inside_the_bars(S, order):
    case = cached_case(S)
    for name in R.CONFIGS:
        for temperature in R.TEMPERATURES:
            got, ref = f32_config(case, name, temperature, order), cached_ref(name, S, temperature)
            assert outside(got, ref) == [False] * 3, (name, temperature, worst(got, ref))
    got, ref = f32_bpr_adj(case, order), cached_ref("bpr", S)
    assert outside(got, ref) == [False] * 3, ("bpr", worst(got, ref))


# ------------------------------------------------------------------------------------------------ (c) seeded defects
@pytest.mark.parametrize("defect,name", [("hit_as_negative", "hits"), ("non_positive_is_hit", "hits"), ("c_on_positive", "logq"),
                                         ("no_log_s", "logq"), ("max_over_masked", "both")])
def test_softmax_defects_leave_the_bars(defect, name):
    hits = 0
    for S in (65, 300):
        for temperature in R.TEMPERATURES:
            hits += any(outside(f32_config(cached_case(S), name, temperature, 0, defect), cached_ref(name, S, temperature)))
    assert hits >= 1, defect


def test_bpr_divided_by_the_kept_count_leaves_the_bars():
    assert sum(any(outside(f32_bpr_adj(cached_case(S), 0, "kept_count"), cached_ref("bpr", S))) for S in (65, 300)) >= 1
    case = cached_case(65)
    ref = cached_ref("bpr", 65)
    no_hits = R.hit_mask(case.indptr, case.cols, case.values, case.items)
    plain = R0.ref_bpr(case.indptr, case.values, case.pred, case.samp, case.go)          # a hit counted as a negative
    assert no_hits.any() and (np.abs(plain.loss - ref.loss) > ref.bar_loss).any()


# ------------------------------------------------------------------------------------------------ (d) the cases
@pytest.mark.parametrize("S", R.SAMPLE_COUNTS)
def test_case_holds_what_it_plants(S):
    case = cached_case(S)
    hits = R.hit_mask(case.indptr, case.cols, case.values, case.items)
    per_user = [int((case.values[case.indptr[u]:case.indptr[u + 1]] > 0).sum()) for u in range(case.n_users)]
    assert per_user == [p for p, _ in R.USERS] and set(per_user) >= {0, 1, 65, 1025}
    assert np.diff(case.indptr)[R.U_ROW1] == 1 and np.diff(case.indptr)[R.U_NONE] == 0
    assert hits[R.U_ALL_HITS].all() and not hits[R.U_NO_HIT].any() and not hits[:2].any()
    assert hits[R.U_ROW1, 0] and (S < 3 or hits[R.U_TRIPLE, :3].all() and len(set(case.items[R.U_TRIPLE, :3])) == 1)
    assert S == 1 or not hits[R.U_NONPOS_ITEM, 0]
    with_zero = R.hit_mask(case.indptr, case.cols, case.values, case.items, count_non_positives=True)
    assert S == 1 or with_zero[R.U_NONPOS_ITEM, 0]
    row = case.cols[case.indptr[R.U_ENDS]:case.indptr[R.U_ENDS + 1]]
    assert case.items[R.U_ENDS, -1] == row[-1] and (S == 1 or case.items[R.U_ENDS, 0] == row[0]) and hits[R.U_ENDS, -1]
    k = case.max_hit_slot
    assert hits[R.U_MAX_HIT, k] and case.samp[R.U_MAX_HIT, k] == case.samp[R.U_MAX_HIT].max()
    assert S == 1 or case.samp[R.U_MAX_HIT, k] - np.delete(case.samp[R.U_MAX_HIT], k).max() > 190
    assert case.log_q.max() == F(-2.0) and case.log_q.min() == F(-14.0)
    assert S < 63 or 0 < hits[3].sum() < S and 0 < hits[10].sum()                            # hits by chance too
    for name in list(R.CONFIGS) + ["bpr"]:
        for temperature in (R.TEMPERATURES if name != "bpr" else [None]):
            ref = cached_ref(name, S, temperature)
            assert all(np.isfinite(x).all() for x in (ref.loss, ref.d_pred, ref.d_samp) + R.bars(ref))
            assert all((b >= 0).all() for b in R.bars(ref))
            if name in ("hits", "both", "both-uniform", "bpr"):
                slots = np.cumsum(case.values > 0) - 1
                mine = slots[case.indptr[R.U_ALL_HITS]:case.indptr[R.U_ALL_HITS + 1]][case.values[case.indptr[R.U_ALL_HITS]:
                                                                                                    case.indptr[R.U_ALL_HITS + 1]] > 0]
                assert (ref.loss[mine] == 0).all() and (ref.bar_loss[mine] == 0).all() and (ref.bar_d_samp[ref.hits] == 0).all()


# ------------------------------------------------------------------------------------------------ (e) the entry points
def test_entry_points_refuse_bad_arguments_before_any_launch():
    from tensorrec_amd import _native
    lib = _native.load()
    p = ctypes.c_void_p(8)

    def ssm_fwd(S=5, t=1.0, first=p, x_item=p, samples=p, use_q=1, no_hits=1, n_items=10, n_users=1, last=p):
        return lib.trec_sampled_softmax_adj_fwd(first, x_item, p, p, p, samples, p, 0.0, n_users, n_items, S, t, use_q, no_hits, p, p, p,
                                                last, None)

    def ssm_bwd(S=5, t=1.0, first=p, x_item=p, samples=p, use_q=1, no_hits=1, n_items=10, n_users=1, last=p):
        return lib.trec_sampled_softmax_adj_bwd(first, x_item, p, p, p, samples, p, 0.0, p, p, p, p, n_users, n_items, S, t, use_q,
                                                no_hits, p, last, None)

    def bpr_fwd(S=5, first=p, x_item=p, samples=p, no_hits=1, n_users=1, last=p, **_):
        return lib.trec_bpr_adj_fwd(first, x_item, p, p, p, samples, n_users, S, no_hits, last, None)

    def bpr_bwd(S=5, first=p, x_item=p, samples=p, no_hits=1, n_users=1, last=p, **_):
        return lib.trec_bpr_adj_bwd(first, x_item, p, p, p, samples, p, n_users, S, no_hits, p, last, None)

    for name, fn in (("trec_sampled_softmax_adj_fwd", ssm_fwd), ("trec_sampled_softmax_adj_bwd", ssm_bwd),
                     ("trec_bpr_adj_fwd", bpr_fwd), ("trec_bpr_adj_bwd", bpr_bwd)):
        for kw in (dict(first=None), dict(last=None)):
            assert fn(**kw) == 1
            assert lib.trec_last_error() == (name + ": null pointer").encode()
        for S in (0, 16385):
            assert fn(S=S) == 1
            assert lib.trec_last_error() == (name + ": n_sampled must be in [1, 16384]").encode()
        assert fn(samples=None) == 1 and b"null samples" in lib.trec_last_error()
        assert fn(x_item=None) == 1 and b"null x_item" in lib.trec_last_error()
        assert fn(n_users=0) == 0                                                       # nothing to do, no launch
        assert fn(n_users=0, samples=None, x_item=None, no_hits=0, use_q=0) == 0        # no option on: neither is needed
    for name, fn in (("trec_sampled_softmax_adj_fwd", ssm_fwd), ("trec_sampled_softmax_adj_bwd", ssm_bwd)):
        assert fn(samples=None, no_hits=0) == 1 and b"null samples" in lib.trec_last_error()
        assert fn(x_item=None, no_hits=0, n_users=0) == 0                               # logQ alone does not need the CSR columns
        assert fn(n_items=0) == 1 and b"n_items" in lib.trec_last_error()
        for t in (0.0, -1.0, float("nan"), float("inf")):
            assert fn(t=t) == 1
            assert lib.trec_last_error() == (name + ": inv_temperature must be finite and > 0").encode()
