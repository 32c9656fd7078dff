"""The WARP kernels (csrc/loss_warp.hip) against the float64 reference of tests/warp_reference.py -- ``first`` and the zero pattern
exactly, the values per element within the bars derived there (tests/test_warp_reference_host.py shows on the CPU that the float32
restatement lies inside them and six seeded defects outside) -- and WARPLossGraph inside a TensorRec fit.

* kernels   S on both sides of the wave-per-user limit with tuning wmrb_wave at its default and at 0 (both forms below 257 samples, the
            workgroup form above); the real-valued family (a positive is left out only under the condition of warp_reference.near, at
            most 0.5 % of a case), the dyadic family, the planted rows, hit removal; exact zeros where the contract asks for them; a
            repeated run bit for bit; ops.warp_loss against the raw entry points;
* model     one captured step against a float64 composition (dot + biases, Euclidean), a graph-replayed fit against the eager fit bit
            for bit, a 30-step fit after which fewer positives still have a violator.

The largest error / bar per family, form and output is kept in RATIOS; with TREC_WARP_RATIOS_OUT=<file> it is written there at the end
(profiles/warp_reference_ratios.json)."""
import functools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import pair_reference as PR
import warp_reference as W
from pair_reference import MODE_DOT, MODE_EUCLID, f64
from test_gpu_pair_kernels import check, dev, tunings

pytestmark = pytest.mark.gpu

RATIOS = {}


@pytest.fixture(scope="module")
def ops():
    from tensorrec_amd import ops as _ops, _native
    _native.require_gpu()
    _native.load()
    yield _ops
    out = os.environ.get("TREC_WARP_RATIOS_OUT")
    if out:
        write_ratios(out)


@pytest.fixture(scope="module")
def N(ops):
    from tensorrec_amd import _native
    return _native


def write_ratios(path):
    """profiles/warp_reference_ratios.json: the ratios of this run"""
    rec = {"what": "largest |result - float64 reference| / bar per family of cases, kernel form (or model configuration) and output over the "
                   "cases of tests/test_gpu_warp_loss.py (bars: tests/warp_reference.py); a bar of 0 asks for equality and records 0",
           "command": "TREC_WARP_RATIOS_OUT=<this file> python -m pytest -m gpu tests/test_gpu_warp_loss.py",
           "ratios": {k: {n: float("%.4g" % v) for n, v in sorted(r.items())} for k, r in sorted(RATIOS.items())}}
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


def held(key, name, got, want, bar, what):
    """check(), with the largest error / bar kept per key and output (a bar of 0 asks for equality)"""
    g, w, b = f64(got).reshape(-1), f64(want).reshape(-1), f64(bar).reshape(-1)
    if g.shape == w.shape and g.size and np.isfinite(g).all():
        err = np.abs(g - w)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = float(np.where(err == 0, 0.0, err / b).max())
        RATIOS.setdefault(key, {})[name] = max(RATIOS.get(key, {}).get(name, 0.0), r)
        print("%s %s %s: largest error / bar %.4g" % (key, what, name, r))
    check(got, want, bar, "%s %s: %s" % (key, what, name))


# ------------------------------------------------------------------------------------------------ kernels
def run_raw(N, case, inter, remove_hits):
    """the two entry points on buffers filled with NaN / -7: whatever is not written shows"""
    P, S = case.pred.size, case.S
    pred, samp, go = dev(case.pred), dev(case.samp), dev(case.go)
    items = dev(case.samples) if remove_hits else None
    loss = torch.full((inter.n_positive,), float("nan"), device="cuda")
    first = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    weight, d_pred = torch.full((P,), float("nan"), device="cuda"), torch.full((P,), float("nan"), device="cuda")
    d_samp = torch.full((case.n_users, S), float("nan"), device="cuda")
    N.call("trec_warp_fwd", N.ptr(inter.indptr), N.ptr(inter.x_item32) if remove_hits else None, N.ptr(inter.pos_slot), N.ptr(pred),
           N.ptr(samp), N.ptr(items), case.n_users, case.n_items, S, 1 if remove_hits else 0, N.ptr(loss), N.ptr(first), N.ptr(weight))
    N.call("trec_warp_bwd", N.ptr(inter.indptr), N.ptr(inter.pos_slot), N.ptr(first), N.ptr(weight), N.ptr(go), case.n_users, S,
           N.ptr(d_pred), N.ptr(d_samp))
    torch.cuda.synchronize()
    return SimpleNamespace(loss=loss.cpu().numpy(), first=first.cpu().numpy(), weight=weight.cpu().numpy(), d_pred=d_pred.cpu().numpy(),
                           d_samp=d_samp.cpu().numpy())


def run_ops(ops, case, inter, remove_hits):
    pt, st = dev(case.pred).requires_grad_(), dev(case.samp).requires_grad_()
    out = ops.warp_loss(pt, st, inter, sample_items=dev(case.samples) if remove_hits else None, remove_accidental_hits=remove_hits)
    out.backward(dev(case.go))
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), pt.grad.cpu().numpy(), st.grad.cpu().numpy()


def check_case(ops, N, family, case, ref, exact_first, remove_hits=False, repeat=False):
    from tensorrec_amd.sparse import Interactions
    inter = Interactions(case.matrix, case.n_users, case.n_items, "cuda")
    assert np.array_equal(inter.indptr.cpu().numpy(), case.indptr) and np.array_equal(inter.values.cpu().numpy(), case.values)
    if remove_hits:
        assert np.array_equal(inter.x_item32.cpu().numpy(), case.x_item)
    S, pos = case.S, case.values > 0
    keep_pos, keep_p, rows, left_out = W.comparable(case, ref)
    if exact_first:                                               # (exact v: nothing is left out, a v of exactly 0 included)
        keep_pos, keep_p, rows = np.ones_like(keep_pos), np.ones_like(keep_p), np.ones_like(rows)
    else:
        assert left_out <= W.MAX_LEFT_OUT, "%.4f of the positives would be left out" % left_out
    no_pos = np.array([not pos[case.indptr[u]:case.indptr[u + 1]].any() for u in range(case.n_users)])
    assert no_pos.sum() >= 2
    for wave in ((1, 0) if S <= 256 else (1,)):                   # (above 256 samples the knob has no effect: the workgroup kernels run)
        with tunings(N, wmrb_wave=wave):
            got = run_raw(N, case, inter, remove_hits)
            via = run_ops(ops, case, inter, remove_hits)
            again = run_raw(N, case, inter, remove_hits) if repeat else None
        form = "wave" if (wave and S <= 256) else "workgroup"
        key, what = "%s %s" % (family, form), "S %d n_items %d" % (S, case.n_items)
        assert np.array_equal(got.first[keep_p], ref.first[keep_p]), "%s %s: first differs at %s" % (
            key, what, np.flatnonzero((got.first != ref.first) & keep_p)[:8])
        assert np.array_equal(got.weight[keep_p] == 0, ref.weight[keep_p] == 0), "%s %s: the zero pattern of weight" % (key, what)
        held(key, "loss", got.loss[keep_pos], ref.loss[keep_pos], ref.bar_loss[keep_pos], what)
        held(key, "d_pred", got.d_pred[keep_p], ref.d_pred[keep_p], ref.bar_d_pred[keep_p], what)
        held(key, "d_samp", got.d_samp[rows], ref.d_samp[rows], ref.bar_d_samp[rows], what)
        assert (got.d_pred[~pos] == 0).all() and (got.first[~pos] == -1).all() and (got.weight[~pos] == 0).all(), \
            "an interaction that is no positive: d_pred / first / weight"
        assert (got.d_samp[no_pos] == 0).all(), "the d_samp row of a user without positives is not exactly 0"
        none = (ref.first == -1) & keep_p
        assert (got.d_pred[none] == 0).all() and (got.loss[none[pos]] == 0).all() and (got.weight[none] == 0).all()
        for name, g, want, keep in (("loss", got.loss, ref.loss, keep_pos), ("d_pred", got.d_pred, ref.d_pred, keep_p),
                                    ("d_samp", got.d_samp, ref.d_samp, rows)):
            assert np.array_equal(g[keep] == 0, want[keep] == 0), "%s %s: the zero pattern of %s" % (key, what, name)
        for name, a, b in zip(("loss", "d_pred", "d_samp"), (got.loss, got.d_pred, got.d_samp), via):
            assert np.array_equal(a, b), "%s %s: ops.warp_loss and the entry points differ in %s" % (key, what, name)
        if again is not None:
            for name in ("loss", "first", "weight", "d_pred", "d_samp"):
                assert np.array_equal(getattr(got, name), getattr(again, name)), "%s %s: two runs differ in %s" % (key, what, name)


@functools.lru_cache(maxsize=4)
def case_and_ref(family, *key):
    """the case and its reference, computed once and left unchanged"""
    case = {"real": W.real_case, "dyadic": W.dyadic_case, "planted": W.planted_case, "hits": W.hits_case}[family](*key)
    return case, W.run_ref(case, remove_hits=family == "hits")


@pytest.mark.parametrize("S", W.SAMPLE_COUNTS)
def test_real_valued_family(ops, N, S):
    """N(0, 1) predictions, a signed go; users with 0 / non-positives only / 1 / 64 / 65 / 1,025 / 2,600 positives, equal samples, a
    positive 100 above and one 100 below every sample ride along at every S"""
    case, ref = case_and_ref("real", S)
    check_case(ops, N, "real", case, ref, exact_first=False)


@pytest.mark.parametrize("S", W.SAMPLE_COUNTS_MANY)
def test_many_positives_and_repeat(ops, N, S):
    """rows of 1,025 and 2,600 positives at S = 40 (wave form: 64 positives per pass; workgroup form: four waves share them, the backward
    pass stages 256) and S = 300 (workgroup form only); every run is made twice and must give the same bits"""
    case, ref = case_and_ref("real", S)
    check_case(ops, N, "real", case, ref, exact_first=False, repeat=True)


@pytest.mark.parametrize("S", W.SAMPLE_COUNTS)
def test_dyadic_family(ops, N, S):
    """multiples of 2^-6 in [-4, 4]: v is exact, ``first`` and every zero pattern must match the reference everywhere"""
    case, ref = case_and_ref("dyadic", S)
    assert W.values_exact(case)
    check_case(ops, N, "dyadic", case, ref, exact_first=True)


@pytest.mark.parametrize("S,n_items,firsts", W.PLANTED, ids=["%d-%d" % p[:2] for p in W.PLANTED])
def test_planted_rows(ops, N, S, n_items, firsts):
    """the first violator at slot 0 / 63 / 64 / 255 / 256 / S - 1, no violator, v = 0 next to v = 2^-20, equal samples, positives far
    above and below; S = 2,000 with n_items = 2,700 (N > 1,349: r = 1, L = 0 with a violator), n_items = 50 (n_items - 1 < N) and
    S = 16,384, the largest; every case also with hit removal and a hit planted one slot before the violator"""
    case, ref = case_and_ref("planted", S, n_items, tuple(firsts))
    check_case(ops, N, "planted", case, ref, exact_first=True, repeat=S == 2000)
    ref_h = W.run_ref(case, remove_hits=True)                     # a hit one slot before the violator: the same first, one trial less
    assert np.array_equal(ref_h.first, ref.first) and ((ref_h.trials < ref.trials).any() or S == 1)
    check_case(ops, N, "planted hits", case, ref_h, exact_first=True, remove_hits=True)
    if S == 2000:
        from tensorrec_amd.sparse import Interactions
        got = run_raw(N, case, Interactions(case.matrix, case.n_users, case.n_items, "cuda"), False)
        dead = (ref.first >= 0) & (ref.trials >= 1350)
        assert dead.sum() >= 4 and (got.first[dead] >= 1349).all() and (got.weight[dead] == 0).all() and (got.d_pred[dead] == 0).all()
        assert (got.loss[dead[case.values > 0]] == 0).all() and (got.d_samp[:, 1349:] == 0).all()


@pytest.mark.parametrize("S", W.SAMPLE_COUNTS + [40])
def test_hit_removal(ops, N, S):
    """remove_accidental_hits: a hit in front of the violator, the only violator a hit, every sample a hit, the column of an interaction
    of value <= 0, repeated ids; rows the wave form holds in registers (<= 64 interactions) and rows it searches in memory"""
    case, ref = case_and_ref("hits", S)
    check_case(ops, N, "hits", case, ref, exact_first=True, remove_hits=True, repeat=S == 40)


# ------------------------------------------------------------------------------------------------ model level
N_USERS, N_ITEMS, S_MODEL = 37, 53, 7
CONFIGS = {"dot-biased-8": (MODE_DOT, True, 8), "euclid-unbiased-5": (MODE_EUCLID, False, 5)}


def model_data():
    rng = np.random.default_rng(17)
    dense = (rng.random((N_USERS, N_ITEMS)) < 0.15).astype(np.float32)
    dense *= np.where(rng.random(dense.shape) < 0.85, 1.0, -1.0).astype(np.float32)
    dense[4, :] = 0                                   # a user without interactions
    dense[9, :] = -np.abs(dense[9, :])                # a user with negative interactions only
    dense[9, 3] = -1.0
    inter = sp.csr_matrix(dense)
    uf = sp.identity(N_USERS, dtype=np.float32, format="csr")
    itf = sp.identity(N_ITEMS, dtype=np.float32, format="csr")
    table = np.stack([rng.choice(N_ITEMS, size=S_MODEL, replace=False) for _ in range(N_USERS)]).astype(np.int32)
    return inter, uf, itf, table


def make_model(T, mode, biased, d, table=None, **kw):
    from tensorrec_amd.loss_graphs import WARPLossGraph
    from tensorrec_amd.prediction_graphs import DotProductPredictionGraph, EuclideanSimilarityPredictionGraph
    pred = DotProductPredictionGraph() if mode == MODE_DOT else EuclideanSimilarityPredictionGraph()
    if table is not None:
        kw["sampler"] = T.ReplaySampler([table])
    return T.TensorRec(n_components=d, prediction_graph=pred, loss_graph=WARPLossGraph(), biased=biased, seed=3, **kw)


def scatter_bar(rows, n_rows, weight):
    out = np.zeros((n_rows,) + weight.shape[1:])
    np.add.at(out, rows, weight)
    return out


def float64_step(w, inter, table, mode, biased, d):
    """(output, float64 value, bar) of one step from the weights ``w``: see test_one_fit_step_against_float64"""
    wants = []
    U, V = w["linear_weights_user_0"], w["linear_weights_item"]
    ub = w["user_feature_biases"].reshape(-1) if biased else None
    ib = w["item_feature_biases"].reshape(-1) if biased else None
    coo = inter.tocoo()                                           # row-major: the serial order of Interactions
    xu, xi = coo.row.astype(np.int64), coo.col.astype(np.int64)
    xus, xis = np.repeat(np.arange(N_USERS), S_MODEL), table.reshape(-1).astype(np.int64)
    sc, scs = PR.ref_pair_scores(U, V, xu, xi, mode, ub, ib), PR.ref_pair_scores(U, V, xus, xis, mode, ub, ib)
    indptr, values = inter.indptr.astype(np.int64), inter.data
    pos = values > 0
    go = np.ones(int(pos.sum()))
    samp = scs.scores.reshape(N_USERS, S_MODEL)
    ref = W.ref_warp(indptr, values, sc.scores, samp, go, N_ITEMS)
    delta_p, delta_s = PR.score_bar(sc, d), PR.score_bar(scs, d).reshape(N_USERS, S_MODEL)
    at_first = np.zeros(values.size)
    ambiguous = []
    for p in np.flatnonzero(pos):
        u, f = xu[p], ref.first[p]
        upto = S_MODEL if f < 0 else f + 1
        v = (1.0 - sc.scores[p]) + samp[u, :upto]
        band = delta_p[p] + delta_s[u, :upto] + W.NEAR * (1.0 + abs(sc.scores[p]) + np.abs(samp[u, :upto]))
        if (np.abs(v) <= band).any():
            ambiguous.append(int(p))
        if f >= 0:
            at_first[p] = delta_p[p] + delta_s[u, f]
    bar_loss = ref.bar_loss + (ref.weight * at_first * (1.0 + 8.0 * PR.U32))[pos]
    wants.append(("pred_serial", sc.scores, delta_p))
    wants.append(("loss", ref.loss, bar_loss))

    ax, ai = np.concatenate([xu, xus]), np.concatenate([xi, xis])
    g, bar_g = np.concatenate([ref.d_pred, ref.d_samp.reshape(-1)]), np.concatenate([ref.bar_d_pred, ref.bar_d_samp.reshape(-1)])
    pg = PR.ref_pair_grads(U, V, ax, ai, g, mode)
    bU, bV, bub, bib = PR.grad_bars(pg, d)
    x, y = f64(U)[ax], f64(V)[ai]
    if mode == MODE_DOT:
        su, sv = np.abs(y), np.abs(x)
    else:
        su = np.where((pg.D >= PR.EPS)[:, None], np.abs(x - y) / np.sqrt(np.maximum(pg.D, 1e-300))[:, None], 0.0)
        sv = su
    bU = bU + scatter_bar(ax, N_USERS, bar_g[:, None] * su)
    bV = bV + scatter_bar(ai, N_ITEMS, bar_g[:, None] * sv)
    wants.append(("d linear_weights_user_0", pg.dU, bU))
    wants.append(("d linear_weights_item", pg.dV, bV))
    if biased:
        bub = bub + scatter_bar(ax, N_USERS, bar_g)
        bib = bib + scatter_bar(ai, N_ITEMS, bar_g)
        wants.append(("d user_feature_biases", pg.dub, bub))
        wants.append(("d item_feature_biases", pg.dib, bib))
    return wants, pg, ref, ambiguous


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_one_fit_step_against_float64(ops, config):
    """One fit_partial step (37 users x 53 items, identity features, so the representations ARE the weight tables; S = 7 replayed samples)
    with the loss vector, the serial predictions and every variable's raw gradient captured, against a float64 composition: scores from
    the weights (pair_reference.ref_pair_scores), warp_reference.ref_warp on those scores with go = 1, pair_reference.ref_pair_grads
    fed with the reference d_pred / d_samp.

    The loss kernels are handed float32 scores that are off by at most delta = pair_reference.score_bar.  A positive's first violator
    is the float64 one unless some sample at or before it has |v| <= delta_p + delta_s + the two-rounding band of v; the weights are
    fixed by the seeds, and the test asserts that no positive is in that case (a condition on the data, as in the kernel tests).  Then
    N_p and L_p are the reference's: d y_p and d y_us keep the kernels' own bars, and loss_p = L_p v_f moves by L_p (delta_p + delta_f)
    more.  The variables' gradients: pair_reference.grad_bars for the sums, plus the pairs' bars carried through |d score / d entry|,
    as in tests/test_gpu_sampled_losses.py."""
    import tensorrec_amd as T
    mode, biased, d = CONFIGS[config]
    inter, uf, itf, table = model_data()
    model = make_model(T, mode, biased, d, table)
    model.build(N_USERS, N_ITEMS)
    w = model.get_weights()
    r2 = np.random.default_rng(7)
    for k in w:                                                   # scores of the order of the margin, so that scans go past slot 0
        scale = 0.1 if k.endswith("biases") else 0.6
        w[k] = (scale * r2.standard_normal(w[k].shape)).astype(np.float32)
    model.set_weights(w)
    w = {k: v.copy() for k, v in model.get_weights().items()}
    model._capture = {}
    model.fit_partial(inter, uf, itf, epochs=1, learning_rate=0.05, alpha=1e-4, n_sampled_items=S_MODEL)
    cap = model._capture
    assert model.last_step_form == "eager" and model.last_step_kernel is None

    key = "model warp %s" % config
    wants, pg, ref, ambiguous = float64_step(w, inter, table, mode, biased, d)
    assert not ambiguous, "positives whose first violator the float32 scores may decide differently: %s" % ambiguous
    assert (ref.first > 0).sum() >= 10 and (ref.first == 0).sum() >= 10
    for name, want, bar in wants:
        got = cap[name] if name in cap else cap["grads"][name[2:]]
        held(key, name, np.asarray(got).reshape(-1), want, bar, "warp")
    assert np.abs(pg.dU).max() > 1e-3 and not pg.dU[4].any() and not cap["grads"]["linear_weights_user_0"][[4, 9]].any()


def disjoint_data(n_users=24, n_pos=3, S=6):
    """every item is the column of at most one pair of a step -- user u's positives are items 9 u .. 9 u + 2, its replayed samples the six
    behind them -- so no sum of the step has more than one term whose order the counting-sort buckets could change (they order a bucket
    by atomic arrival): graph replays and eager steps can be compared bit for bit.  User 5 has no interaction, user 7 a negative one."""
    per = n_pos + S
    rows, cols, vals = [], [], []
    for u in range(n_users):
        if u == 5:
            continue
        for j in range(n_pos):
            rows.append(u)
            cols.append(per * u + j)
            vals.append(-1.0 if (u == 7 and j == 1) else 1.0)
    n_items = per * n_users
    inter = sp.csr_matrix((np.array(vals, np.float32), (rows, cols)), shape=(n_users, n_items))
    table = np.stack([per * u + n_pos + np.arange(S) for u in range(n_users)]).astype(np.int32)
    return inter, sp.identity(n_users, dtype=np.float32, format="csr"), sp.identity(n_items, dtype=np.float32, format="csr"), table


def test_hip_graph_replay_equals_eager_steps_bit_for_bit(ops):
    """a fit whose later steps are HIP-graph replays reports last_step_form "graph", takes no one-pass kernel and ends with the weights
    of the all-eager fit, bit for bit (disjoint_data: no sum of the step depends on the order inside an item's bucket)"""
    import tensorrec_amd as T
    inter, uf, itf, table = disjoint_data()
    out = []
    for graphs in (True, False):
        model = make_model(T, MODE_DOT, True, 8, table, hip_graphs=graphs)
        model.fit(inter, uf, itf, epochs=6, learning_rate=0.05, n_sampled_items=table.shape[1])
        assert model.last_step_form == ("graph" if graphs else "eager") and model.last_step_kernel is None
        out.append((model.get_weights(), model._opt_step, model._sample_step))
    (wa, oa, sa), (wb, ob, sb) = out
    assert (oa, sa) == (ob, sb) == (6, 6)
    for k in wa:
        assert np.array_equal(wa[k], wb[k]), k
    assert any(np.abs(wa[k]).max() > 0 for k in wa)


def test_thirty_steps_leave_fewer_violators(ops):
    """a 30-step fit on a small planted-cluster set: the share of positives that still have a violator among ONE fixed table of samples
    (ops.warp_loss on the model's predictions: loss_p > 0 iff a violator exists, the rank weight being > 0 at these sizes) goes down"""
    import tensorrec_amd as T
    from tensorrec_amd.sparse import Interactions
    from tensorrec_amd.synth import planted_cluster_interactions
    n_users, n_items, S = 200, 300, 10
    train, _, _, _ = planted_cluster_interactions(n_users, n_items, n_clusters=8, per_user=10, seed=0, device="cuda")
    uf = sp.identity(n_users, dtype=np.float32, format="csr")
    itf = sp.identity(n_items, dtype=np.float32, format="csr")
    table = np.stack([np.random.default_rng(100 + u).choice(n_items, size=S, replace=False) for u in range(n_users)])
    inter = Interactions(train, n_users, n_items, "cuda")
    coo = train.tocoo()
    assert (n_items - 1) // S > 1

    def share(model):
        scores = np.asarray(model.predict(uf, itf), dtype=np.float32)
        loss = ops.warp_loss(dev(scores[coo.row, coo.col]), dev(scores[np.arange(n_users)[:, None], table]), inter)
        return float((loss > 0).float().mean().item())

    model = make_model(T, MODE_DOT, True, 16)
    model.build(n_users, n_items)
    before = share(model)
    for _ in range(30):
        model.fit_partial(train, uf, itf, epochs=1, learning_rate=0.05, n_sampled_items=S)
    after = share(model)
    assert model.last_step_kernel is None
    print("share of positives with a violator: %.4f before the fit, %.4f after 30 steps" % (before, after))
    assert 0.0 <= after < before <= 1.0, (before, after)
